// Engine: state layout, device buffers and covariance operations.
#include <sys/stat.h>

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "engine.h"

namespace uvhp {

// ---- Type::update family ----
void Var::update(const double *dx) {
  if (kind == V_IMU || kind == V_POSE || kind == V_QUAT || kind == V_AUX_QUAT) {
    quat_boxplus(val, dx);
    for (int i = 3; i < size; i++) val[i + 1] += dx[i];
  } else {
    for (int i = 0; i < size; i++) val[i] += dx[i];
  }
}

// Landmark::get_xyz (Landmark.cpp:26-63); representation ids of LandmarkRepresentation.h:38
// (the shared statement of landmark_rep.h, which the device's landmark read uses too)
void Var::xyz(bool getfej, double *o) const { landmark_get_xyz(rep, val, fej, uvn0, getfej, o); }
void Var::set_xyz(const double *p, bool isfej) {
  landmark_set_from_xyz(rep, p, isfej ? fej : val, isfej ? uvn0_fej : uvn0);
}

// ---- Feature (Feature.cpp:26-111) ----
void MeasList::keep_if_valid(const std::vector<double> &valid) {
  size_t w = b;
  for (size_t i = b; i < v.size(); i++)
    if (std::binary_search(valid.begin(), valid.end(), v[i].t)) v[w++] = v[i];
  v.resize(w);
  if (v.size() == b) clear();
  recache();
}
// Feature::clean_old_measurements (Feature.cpp:37-60): keep the measurements at the given (sorted) times
void Feature::clean_old_measurements(const std::vector<double> &valid) {
  for (auto &c : tracks) c.m.keep_if_valid(valid);
}
// Feature::clean_older_measurements (Feature.cpp:85-104): drop every measurement at or before t.  A camera's
// measurements of an in-order stream form a prefix, found by binary search (MeasList::drop_through).
void Feature::clean_older_measurements(double t) {
  for (auto &c : tracks) c.m.drop_through(t);
}

static VarP mk(VKind k, int size, int vlen) { return std::make_shared<Var>(k, size, vlen); }

// State::State (State.cpp:28-166) + UVioManager ctor (UVioManager.cpp:26-58)
Engine::Engine(const uvio_hp_options_t &o, int device) : o_(o), device_(device) {
  if (o_.num_cameras < 1 || o_.num_cameras > UVIO_HP_MAX_CAMS) throw HpError(UVIO_HP_E_ARG, "num_cameras out of range");
  g_track_reserve.store(std::max(8, o_.max_clone_size + 4), std::memory_order_relaxed);
  // configurations the reference accepts but this build does not implement fail here, loudly
  if (!o_.use_klt) throw HpError(UVIO_HP_E_CONFIG, "use_klt: false (TrackDescriptor / ORB) is not implemented");
  if (o_.use_aruco) throw HpError(UVIO_HP_E_CONFIG, "use_aruco: true (TrackAruco) is not implemented");
  if (o_.histogram_method < 0 || o_.histogram_method > 2)
    throw HpError(UVIO_HP_E_CONFIG, "histogram_method: 0 (NONE), 1 (HISTOGRAM) or 2 (CLAHE)");
  if (o_.feat_rep_msckf < 0 || o_.feat_rep_msckf > 5)
    throw HpError(UVIO_HP_E_CONFIG, "feat_rep_msckf: unknown landmark representation");
  if (o_.feat_rep_slam < 0 || o_.feat_rep_slam > 5)
    throw HpError(UVIO_HP_E_CONFIG, "feat_rep_slam: unknown landmark representation");
  currid_ = 4 * (size_t)o_.max_aruco_features + 1;  // TrackBase::currid (TrackBase.cpp:34)
  int cur = 0;
  imu_ = mk(V_IMU, 15, 16);
  imu_->val[3] = imu_->fej[3] = 1;
  imu_->id = cur;
  vars_.push_back(imu_);
  cur += 15;
  dw_ = mk(V_VEC, 6, 6);
  da_ = mk(V_VEC, 6, 6);
  tg_ = mk(V_VEC, 9, 9);
  qg_ = mk(V_QUAT, 3, 4);
  qa_ = mk(V_QUAT, 3, 4);
  for (int k = 0; k < 6; k++) dw_->val[k] = dw_->fej[k] = o_.imu_dw[k], da_->val[k] = da_->fej[k] = o_.imu_da[k];
  for (int k = 0; k < 9; k++) tg_->val[k] = tg_->fej[k] = o_.imu_tg[k];
  for (int k = 0; k < 4; k++) qg_->val[k] = qg_->fej[k] = o_.q_GYROtoIMU[k], qa_->val[k] = qa_->fej[k] = o_.q_ACCtoIMU[k];
  if (o_.do_calib_imu_intrinsics) {
    for (auto &v : {dw_, da_}) {
      v->id = cur;
      vars_.push_back(v);
      cur += v->size;
    }
    if (o_.do_calib_imu_g_sensitivity) {
      tg_->id = cur;
      vars_.push_back(tg_);
      cur += 9;
    }
    VarP q = (o_.imu_model == 0) ? qg_ : qa_;
    q->id = cur;
    vars_.push_back(q);
    cur += 3;
  }
  calib_dt_ = mk(V_VEC, 1, 1);
  calib_dt_->val[0] = calib_dt_->fej[0] = o_.calib_camimu_dt;
  if (o_.do_calib_camera_timeoffset) {
    calib_dt_->id = cur;
    vars_.push_back(calib_dt_);
    cur += 1;
  }
  for (int i = 0; i < o_.num_cameras; i++) {
    VarP pose = mk(V_POSE, 6, 7), intr = mk(V_VEC, 8, 8);
    const uvio_hp_camera_t &c = o_.cams[i];
    for (int k = 0; k < 4; k++) pose->val[k] = pose->fej[k] = c.q_ItoC[k];
    for (int k = 0; k < 3; k++) pose->val[4 + k] = pose->fej[4 + k] = c.p_IinC[k];
    for (int k = 0; k < 8; k++) intr->val[k] = intr->fej[k] = c.intrinsics[k];
    calib_pose_.insert({(size_t)i, pose});
    calib_intr_.insert({(size_t)i, intr});
    cams_[i].model = c.model;
    cams_[i].w = c.width;
    cams_[i].h = c.height;
    for (int k = 0; k < 8; k++) cams_[i].v[k] = c.intrinsics[k];
    if (o_.do_calib_camera_pose) {
      pose->id = cur;
      vars_.push_back(pose);
      cur += 6;
    }
    if (o_.do_calib_camera_intrinsics) {
      intr->id = cur;
      vars_.push_back(intr);
      cur += 8;
    }
  }
  N_ = cur;
  chi2_table_ = std::vector<double>(1000, 0.0);
  alloc_device();
  // initial covariance (State.cpp:133-165): built once on the host, then resident on the device
  std::vector<double> Ph((size_t)N_ * N_, 0.0);
  for (int i = 0; i < N_; i++) Ph[(size_t)i * N_ + i] = 1e-6;
  auto setd = [&](int id, int n, double v) {
    for (int k = 0; k < n; k++) Ph[(size_t)(id + k) * N_ + id + k] = v;
  };
  if (o_.do_calib_imu_intrinsics) {
    setd(dw_->id, 6, 0.005 * 0.005);
    setd(da_->id, 6, 0.008 * 0.008);
    if (o_.do_calib_imu_g_sensitivity) setd(tg_->id, 9, 0.005 * 0.005);
    setd((o_.imu_model == 0 ? qg_ : qa_)->id, 3, 0.005 * 0.005);
  }
  if (o_.do_calib_camera_timeoffset) setd(calib_dt_->id, 1, 0.01 * 0.01);
  for (int i = 0; i < o_.num_cameras; i++) {
    if (o_.do_calib_camera_pose) {
      setd(calib_pose_.at(i)->id, 3, 0.005 * 0.005);
      setd(calib_pose_.at(i)->id + 3, 3, 0.015 * 0.015);
    }
    if (o_.do_calib_camera_intrinsics) {
      setd(calib_intr_.at(i)->id, 4, 1.0);
      setd(calib_intr_.at(i)->id + 4, 4, 0.005 * 0.005);
    }
  }
  upload_P_full(Ph, N_);
  if (o_.record_timing_information) {
    // VioManager.cpp:105-122: the old file is replaced, its directory created
    std::string path(o_.record_timing_filepath);
    std::remove(path.c_str());
    for (size_t k = 1; k < path.size(); k++)
      if (path[k] == '/') mkdir(path.substr(0, k).c_str(), 0755);
    timing_csv_ = std::fopen(path.c_str(), "a");
    if (!timing_csv_) throw HpError(UVIO_HP_E_CONFIG, "record_timing_filepath: cannot open " + path);
    std::fprintf(timing_csv_, "# timestamp (sec),tracking,propagation,msckf update,");
    if (o_.max_slam_features > 0) std::fprintf(timing_csv_, "slam update,slam delayed,");
    std::fprintf(timing_csv_, "re-tri & marg,total\n");
  }
  // uvio
  p_IinU_ = mk(V_VEC, 3, 3);
  for (int k = 0; k < 3; k++) p_IinU_->val[k] = p_IinU_->fej[k] = o_.p_IinU[k];
  if (o_.use_uwb) {
    if (o_.do_calib_uwb_extrinsics) {
      std::vector<double> HR(9, 0.0), HL(9, 0.0), R(9, 0.0), res(3, 0.0);
      for (int k = 0; k < 3; k++) HL[4 * k] = 1.0, R[4 * k] = o_.prior_uwb_imu_cov;
      initialize_invertible_host(p_IinU_, {{imu_->id, 3}}, HR, HL, R, res);
      for (int k = 0; k < 3; k++) p_IinU_->val[k] = p_IinU_->fej[k] = o_.p_IinU[k];
    }
    if (o_.n_anchors > 0) init_anchors(o_.n_anchors, o_.anchors);
  }
}

Engine::~Engine() {
  if (timing_csv_) std::fclose(timing_csv_);
  hipSetDevice(device_);  // the members' destructors run after this body: every free happens on this device
  if (shard_.nccl) rccl_comm_destroy(shard_.nccl);  // before the stream it used
  tracker_.reset();
}

// Capacities from the config (DESIGN.md "Data layout"): P is sized for the largest state the
// config can reach (IMU + intrinsics + dt + cams + (max_clones+1) clones + max_slam landmarks +
// anchors + p_IinU), so appends / deletions never reallocate.
void Engine::alloc_device() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_)
    throw HpError(UVIO_HP_E_DEVICE, "no HIP device " + std::to_string(device_));
  HP_HIP(hipSetDevice(device_));
  d_.stream = Stream::create();
  d_.aux = Stream::create();
  d_.ev_aux_in = Event::create();
  d_.ev_aux_out = Event::create();
  d_.copy = Stream::create();
  d_.ev_copy = Event::create();
  kprof_.stream = d_.stream;
  rt_.copied = Event::create();
  d_.ekf.kp = &kprof_;
  int C = o_.max_clone_size + 2;
  int K = o_.num_cameras;
  // (max_aux_dim: room for the caller's own variables, uvio_hp_aux_add; 0 leaves every size as it was)
  int cap = N_ + 6 * C + 3 * std::max(o_.max_slam_features, 0) + 5 * UVIO_HP_MAX_ANCHORS + 3 + 8 +
            std::max(o_.max_aux_dim, 0);
  cap = (cap + 7) / 8 * 8;
  d_.ldp = cap;
  d_.P = DevBuf<double>((size_t)cap * cap);
  d_.P2 = DevBuf<double>((size_t)cap * cap);
  d_.T = DevBuf<double>((size_t)cap * 64);
  d_.Phi = DevBuf<double>(64 * 64);
  d_.Q = DevBuf<double>(64 * 64);
  d_.dnc = DevBuf<double>(8);
  d_.iold = DevBuf<int>(256);
  // update batch capacities
  int maxf = std::max(o_.max_msckf_in_update, 1);
  maxf = std::min(maxf, 4096);
  maxf = std::max(maxf, std::max(o_.max_slam_in_update, o_.max_slam_features));
  maxf = std::min(std::max(maxf, 64), 8192);
  d_.max_feat = maxf;
  int meas_per_feat = std::min(C * K, kMaxMeasPerFeat);
  d_.max_meas_total = maxf * meas_per_feat;
  d_.max_vars_total = maxf * kMaxVarsPerFeat;
  d_.max_rows = maxf * 2 * meas_per_feat;
  d_.max_ncol = cap + 1;
  d_.ldh = (d_.max_ncol + 7) / 8 * 8;
  d_.chi2 = DevBuf<double>(1000);
  d_.H = DevBuf<double>((size_t)d_.max_rows * d_.ldh);
  d_.Tall = DevBuf<double>((size_t)d_.max_rows * d_.ldh);
  int maxch = std::max((d_.max_rows + 511) / 512 + 1, gram_num_chunks(2048) + 1);  // 512- or 64-row chunks
  d_.partials = DevBuf<double>((size_t)maxch * d_.max_ncol * d_.max_ncol);
  d_.R = DevBuf<double>((size_t)2 * d_.max_ncol * d_.ldh);
  d_.hidx_pre = DevBuf<int>((size_t)DeviceBufs::kPreSlots * d_.max_ncol);
  d_.hidx_pre_h = PinBuf<int>((size_t)DeviceBufs::kPreSlots * d_.max_ncol);
  for (auto &e : d_.ev_pre) e = Event::create();
  int rmax = std::max(d_.max_ncol, kMaxEkfRows);
  d_.ekf.M = d_.ekf_M = DevBuf<double>((size_t)cap * rmax);
  d_.ekf.W = d_.ekf_W = DevBuf<double>((size_t)cap * rmax);
  d_.ekf.S = d_.ekf_S = DevBuf<double>((size_t)5 * rmax * rmax);
  d_.ekf.y = d_.ekf_y = DevBuf<double>(rmax);
  d_.ekf.M3 = d_.ekf_M3 = DevBuf<double>((size_t)cap * 3);
  d_.ekf.Dinv = d_.ekf_Dinv = DevBuf<double>((size_t)(rmax / 16 + 1) * 256);
  d_.dx_bytes = sizeof(double) * (cap + 16);
  // One chain holds the MSCKF batch (at most maxf features, one region), the SLAM chunks (a result slot per
  // landmark, at most a region each) and the delayed initialization's two passes (two slots and one region per
  // candidate).  Landmarks and candidates each own 3 columns of P, so there are at most cap / 3 of them together:
  // the chain's covariance check (N0 + 3 K > ldp) always binds before its region or result-slot checks.
  const int max3 = cap / 3;
  d_.fout_cap = maxf + 2 * max3 + 64;
  d_.chain_k = max3 + 4;
  d_.chain_stride = (size_t)cap + 16;
  // [chain regions (reversed) | dx block (neg, dx) | fout] on the device and mirrored in pinned memory
  const size_t reg_bytes = sizeof(double) * d_.chain_k * d_.chain_stride;
  const size_t res_bytes = reg_bytes + d_.dx_bytes + sizeof(DFeatOut) * d_.fout_cap;
  d_.chain = DevBuf<char>(res_bytes);
  HP_HIP(hipMemset(d_.chain, 0, res_bytes));
  d_.dxneg = (double *)((char *)d_.chain + reg_bytes);
  d_.fout = (DFeatOut *)((char *)d_.dxneg + d_.dx_bytes);
  d_.acc = DevBuf<int>(4);
  d_.shard = DevBuf<double>((size_t)d_.max_ncol * d_.max_ncol + 2);
  d_.ekf.neg = (int *)d_.dxneg;
  d_.ekf.dx = d_.dxneg + 1;
  d_.chain_host = PinBuf<char>(res_bytes + 64);
  // chi2 table: boost::math::quantile(chi_squared(dof), 0.95) for dof 1..999 (UpdaterMSCKF.cpp:52-55)
  for (int i = 1; i < 1000; i++) chi2_table_[i] = chi2_quantile95(i);
  HP_HIP(hipMemcpy(d_.chi2, chi2_table_.data(), 1000 * sizeof(double), hipMemcpyHostToDevice));
  char *pb = (char *)d_.chain_host + reg_bytes;
  d_.neg_host = (int *)pb;  // same layout as dxneg
  d_.dx_host = (double *)(pb + sizeof(double));
  d_.fout_host = (DFeatOut *)(pb + d_.dx_bytes);
  // the chain's state blob: a clone owns 6 columns of P, so there are at most cap / 6 of them
  const int maxcl = cap / 6;
  d_.frame_bytes = sizeof(DClone) * maxcl + sizeof(DCam) * UVIO_HP_MAX_CAMS + sizeof(DPoseVal) * (maxcl + UVIO_HP_MAX_CAMS) +
                   sizeof(double) * cap + 1024;
  d_.frame = DevBuf<char>(d_.frame_bytes);
  // upload staging ring (batch tables, Phi / Q, column maps): one full update batch's tables and some slack
  const size_t batch_bytes =
      sizeof(DFeat) * maxf + sizeof(DMeas) * d_.max_meas_total + sizeof(DVar) * d_.max_vars_total +
      sizeof(DClone) * (C + 4) + sizeof(DCam) * UVIO_HP_MAX_CAMS + sizeof(int) * (d_.max_ncol + d_.max_rows) +
      sizeof(double) * (cap + 16) + sizeof(DFeatOut) * (maxf + 3 * std::max(o_.max_slam_features, 0) + 64) +
      sizeof(double) * 16 + 4096;
  d_.stg_cap = batch_bytes + 2 * 64 * 64 * sizeof(double) + 64 * 1024;
  // test hook: a smaller ring recycles every few batches (tests/test_gpu_configs.py staging test)
  if (const char *e = std::getenv("UVIO_HP_STAGE_BYTES")) d_.stg_cap = std::min(d_.stg_cap, (size_t)std::atoll(e));
  if (const char *e = std::getenv("UVIO_HP_NO_PREDETECT")) predetect_on_ = e[0] != '1';
  d_.stg_h = PinBuf<char>(d_.stg_cap);
  d_.stg_d = DevBuf<char>(d_.stg_cap);
  d_.mchain_stride = (size_t)d_.ldp + kChainHeader;
  d_.mchain_reg = DevBuf<unsigned char>(kChainMaxSteps * d_.mchain_stride * sizeof(double));
  d_.mchain_host = PinBuf<double>(kChainMaxSteps * d_.mchain_stride);
  d_.mchain_row = DevBuf<DChainRow>(kChainMaxSteps);
}

void Engine::upload_P_full(const std::vector<double> &Ph, int N) {
  HP_HIP(hipMemcpy2DAsync(d_.P, sizeof(double) * d_.ldp, Ph.data(), sizeof(double) * N, sizeof(double) * N, N,
                          hipMemcpyHostToDevice, d_.stream));
  ++p_epoch_;
  dev_sync();
}
void Engine::download_P(std::vector<double> &Ph) {
  Ph.assign((size_t)N_ * N_, 0.0);
  if (N_ == 0) return;
  HP_HIP(hipMemcpy2DAsync(Ph.data(), sizeof(double) * N_, d_.P, sizeof(double) * d_.ldp, sizeof(double) * N_, N_,
                          hipMemcpyDeviceToHost, d_.stream));
  dev_sync();
}
void Engine::get_cov(double *out, int ld) {
  HP_HIP(hipMemcpy2DAsync(out, sizeof(double) * ld, d_.P, sizeof(double) * d_.ldp, sizeof(double) * N_, N_,
                          hipMemcpyDeviceToHost, d_.stream));
  dev_sync();
}

// A ring: tables are appended after the last flushed one and the ring restarts only when full (after
// a stream sync), so a staged table stays valid on the device until many later launch groups.
void *Engine::stage_bytes(const void *src, size_t bytes) {
  const size_t need = (bytes + 255) / 256 * 256;
  if (need > d_.stg_cap) throw HpError(UVIO_HP_E_CAPACITY, "upload staging exhausted");
  if (d_.stg_used + need > d_.stg_cap) {
    stage_flush();
    dev_sync();
    d_.stg_used = d_.stg_flushed = 0;
    d_.stg_epoch++;
    timing_.stage_restarts++;
  }
  if (bytes) std::memcpy(d_.stg_h + d_.stg_used, src, bytes);
  void *dev = d_.stg_d + d_.stg_used;
  d_.stg_used += need;
  return dev;
}

void *Engine::stage_reserve(size_t bytes, void **host) {
  const size_t need = (bytes + 255) / 256 * 256;
  if (need > d_.stg_cap) throw HpError(UVIO_HP_E_CAPACITY, "upload staging exhausted");
  if (d_.stg_used + need > d_.stg_cap) {
    stage_flush();
    dev_sync();
    d_.stg_used = d_.stg_flushed = 0;
    d_.stg_epoch++;
    timing_.stage_restarts++;
  }
  *host = d_.stg_h + d_.stg_used;
  void *dev = d_.stg_d + d_.stg_used;
  d_.stg_used += need;
  return dev;
}

// With kernels still queued on the main stream the upload goes out on the copy stream and the main stream waits
// on its event: enqueued on the main stream the transfer started only after every kernel queued before it (the
// chain's SLAM tables behind the MSCKF update), and its ~15-20 us from start to completion showed as an idle
// gap before the next launch.  On an idle main stream the copy goes there directly (the cross-stream wait only
// adds latency then).  The ring region is not read by anything queued earlier (reused only after a restart,
// which syncs).  The one exception is a copy queued on the main stream after a restart that still reads the
// previous epoch's bytes (the chain's blob, engine_chain.cpp): its caller passes on_main, so the upload of the
// new epoch, which may overwrite those bytes, is ordered behind the copy.
void Engine::stage_flush(bool on_main) {
  if (d_.stg_used == d_.stg_flushed) return;
  const bool idle = on_main || hipStreamQuery(d_.stream) == hipSuccess;
  HP_HIP(hipMemcpyAsync(d_.stg_d + d_.stg_flushed, d_.stg_h + d_.stg_flushed, d_.stg_used - d_.stg_flushed,
                        hipMemcpyHostToDevice, idle ? d_.stream : d_.copy));
  if (!idle) {
    HP_HIP(hipEventRecord(d_.ev_copy, d_.copy));
    HP_HIP(hipStreamWaitEvent(d_.stream, d_.ev_copy, 0));
  }
  d_.stg_flushed = d_.stg_used;
}

void Engine::dev_sync() {
  auto t0 = std::chrono::steady_clock::now();
  spin_sync(d_.stream);
  timing_.sync_wait += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  timing_.device_syncs++;
  if (kprof_.on) kprof_.harvest(true);
}

// cumulative per-class kernel statistics since the timing was switched on (flush: wait for the device
// so every recorded launch is counted)
void Engine::kernel_stats(bool flush, uvio_hp_kstat_t *out, int cap, int *n) {
  static const struct {
    const char *name, *kernels;
    int bound;
  } info[KC_COUNT] = {
      {"feature", "k_feature", 1},
      {"chi2", "k_gather_pcan,k_gemm_HPg,k_gemm_HPg_tiled,k_chi2_S,k_chi2_S2,k_chi2,k_chi2_small", 1},
      {"gram", "k_gram,k_gram_mfma", 1},
      {"ekf_update", "k_ekf_MS,k_ekf_fact,k_ekf_WP,k_gram_reduce,k_info_cholP,k_gemm_mfma,k_info_cholZ,k_trinv16,"
                     "k_trsm_lt,k_info_P,k_di_M,k_di_S,k_info_split1,k_info_split_schur,k_info_split3,k_info_split_out",
       1},
      {"ldl", "k_ekf_fact", 1},
      {"lk", "k_lk", 0},
      {"pyramid", "k_hist_multi,k_clahe_lut,k_pyr_pair", 0},
      {"fast", "k_fast_score,k_fast_select", 0},
      {"subpix", "k_subpix", 0},
  };
  // the tracker's detection stream (predetect on the worker thread) keeps its own event pairs
  const KProf *pre = nullptr;
  if (flush) {
    HP_HIP(hipStreamSynchronize(d_.stream));
    kprof_.harvest(true);
    if (tracker_) pre = &tracker_->pre_prof();
    // LK bytes are counted on the device by both streams' timed launches (LkSlots::bytes), never credited
    if (tracker_) kprof_.bytes[KC_LK] = (double)tracker_->lk_bytes();
  }
  *n = KC_COUNT;
  for (int k = 0; k < KC_COUNT && k < cap; k++) {
    uvio_hp_kstat_t &o = out[k];
    std::memset(&o, 0, sizeof(o));
    std::snprintf(o.name, sizeof(o.name), "%s", info[k].name);
    std::snprintf(o.kernels, sizeof(o.kernels), "%s", info[k].kernels);
    o.bound = info[k].bound;
    o.launches = kprof_.launches[k] + (pre ? pre->launches[k] : 0);
    o.seconds = kprof_.secs[k] + (pre ? pre->secs[k] : 0.0);
    o.flops = kprof_.flops[k] + (pre ? pre->flops[k] : 0.0);
    o.bytes = kprof_.bytes[k] + (pre ? pre->bytes[k] : 0.0);
  }
}

// regions 0 .. nreg-1 of the frame chain, the dx block and the first fo per-feature results: one contiguous span
// of the results block (DeviceBufs::region_dev), one copy
void Engine::chain_results_copy(int nreg, int fo) {
  if (nreg <= 0 && fo <= 0) return;
  const char *d0 = (const char *)d_.region_dev(std::max(nreg, 0) - 1);
  const char *d1 = (const char *)(d_.fout + std::max(fo, 0));
  char *h0 = (char *)d_.region_host(std::max(nreg, 0) - 1);
  HP_HIP(hipMemcpyAsync(h0, d0, (size_t)(d1 - d0), hipMemcpyDeviceToHost, d_.stream));
}

void Engine::read_dx(const char *who) {
  HPROF("read_dx");
  // [count | dx (N)]
  HP_HIP(hipMemcpyAsync(d_.neg_host, d_.dxneg, sizeof(double) * (3 + (size_t)N_), hipMemcpyDeviceToHost, d_.stream));
  dev_sync();
  if (*d_.neg_host > 0) throw HpError(UVIO_HP_E_NUMERIC, std::string(who) + ": negative covariance diagonal");
}

// StateHelper::EKFPropagation on the device (StateHelper.cpp:36-114).  The new block is rows
// s0 .. s0+p-1, or the rows listed in `rows` (several variables at once, block-row Phi).
void Engine::cov_propagate(int s0, int p, const std::vector<int> &iold, const std::vector<double> &Phi,
                           const std::vector<double> &Q, const std::vector<int> *rows) {
  int q = (int)iold.size();
  if (p > 64 || q > 256) throw HpError(UVIO_HP_E_CAPACITY, "propagation block too large");
  const double *dPhi = stage(Phi.data(), (size_t)p * q);
  const double *dQ = stage(Q.data(), (size_t)p * p);
  const int *diold = stage(iold.data(), (size_t)q);
  const int *drows = rows ? stage(rows->data(), rows->size()) : nullptr;
  stage_flush();
  launch_cov_propagate(d_.stream, d_.P, d_.ldp, N_, s0, p, diold, q, dPhi, dQ, d_.T, drows);
  ++p_epoch_;
}

void Engine::check_neg_diag(const char *who) {
  HP_HIP(hipMemsetAsync(d_.ekf.neg, 0, sizeof(int), d_.stream));
  launch_check_diag(d_.stream, d_.P, d_.ldp, N_, d_.ekf.neg);
  HP_HIP(hipMemcpyAsync(d_.neg_host, d_.ekf.neg, sizeof(int), hipMemcpyDeviceToHost, d_.stream));
  dev_sync();
  if (*d_.neg_host > 0) throw HpError(UVIO_HP_E_NUMERIC, std::string(who) + ": negative covariance diagonal");
}

// cov_propagate of the IMU block (contiguous rows s0 ..) followed by clone_imu_pose, as ONE launch when the
// propagation is small (launch_prop_clone); false when it did nothing (the caller takes the two-step path)
bool Engine::cov_propagate_clone(int s0, int p, const std::vector<int> &iold, const std::vector<double> &Phi,
                                 const std::vector<double> &Q, bool do_dt, const double *ddnc) {
  const int q = (int)iold.size();
  if (!prop_clone_fits(N_, p, q) || N_ + 6 > d_.ldp) return false;
  const double *dPhi = stage(Phi.data(), (size_t)p * q);
  const double *dQ = stage(Q.data(), (size_t)p * p);
  const int *diold = stage(iold.data(), (size_t)q);
  stage_flush();
  if (!launch_prop_clone(d_.stream, d_.P, d_.ldp, N_, s0, p, diold, q, dPhi, dQ, d_.T, imu_->id,
                         do_dt ? calib_dt_->id : 0, do_dt ? ddnc : d_.dnc, do_dt ? 1 : 0))
    throw HpError(UVIO_HP_E_CAPACITY, "fused propagation refused after the size check");
  ++p_epoch_;
  return true;
}

// StateHelper::clone(imu->pose()) + augment_clone (StateHelper.cpp:341-391, 579-616)
VarP Engine::clone_imu_pose(const double *dnc, bool do_dt, const double *staged) {
  if (N_ + 6 > d_.ldp) throw HpError(UVIO_HP_E_CAPACITY, "covariance capacity exceeded");
  const double *ddnc = d_.dnc;
  if (do_dt) {
    ddnc = staged;  // already on the device (staged and flushed by the caller)
    if (!ddnc) {
      ddnc = stage(dnc, 6);
      stage_flush();
    }
  }
  launch_clone(d_.stream, d_.P, d_.ldp, N_, imu_->id, do_dt ? calib_dt_->id : 0, ddnc, do_dt ? 1 : 0);
  ++p_epoch_;
  return add_clone_var();
}

// the clone's host variable (its covariance rows / columns N_ .. N_+5 are written on the device)
VarP Engine::add_clone_var() {
  VarP pose = mk(V_POSE, 6, 7);
  for (int k = 0; k < 7; k++) pose->val[k] = imu_->val[k], pose->fej[k] = imu_->fej[k];
  pose->id = N_;
  N_ += 6;
  vars_.push_back(pose);
  return pose;
}

// StateHelper::marginalize (StateHelper.cpp:271-339)
void Engine::marginalize(const VarP &m) {
  int m0 = m->id, ms = m->size;
  launch_marginalize(d_.stream, d_.P, d_.P2, d_.ldp, N_, m0, ms);
  std::swap(d_.P, d_.P2);
  ++p_epoch_;
  std::vector<VarP> keep;
  for (auto &v : vars_)
    if (v != m) {
      if (v->id > m0) v->id -= ms;
      keep.push_back(v);
    }
  vars_ = keep;
  m->id = -1;
  N_ -= ms;
}

void Engine::marginalize_many(const std::vector<VarP> &ms) {
  if (ms.empty()) return;
  if (ms.size() == 1) {
    marginalize(ms[0]);
    return;
  }
  std::vector<uint8_t> gone((size_t)N_, 0);
  for (const auto &m : ms)
    for (int k = 0; k < m->size; k++) gone[(size_t)(m->id + k)] = 1;
  std::vector<int> src, before((size_t)N_ + 1, 0);
  src.reserve((size_t)N_);
  for (int i = 0; i < N_; i++) {
    before[(size_t)i + 1] = before[(size_t)i] + gone[(size_t)i];
    if (!gone[(size_t)i]) src.push_back(i);
  }
  const int Nn = (int)src.size();
  const int *dsrc = stage(src.data(), src.size());
  stage_flush();
  launch_marginalize_multi(d_.stream, d_.P, d_.P2, d_.ldp, Nn, dsrc);
  std::swap(d_.P, d_.P2);
  ++p_epoch_;
  std::vector<VarP> keep;
  keep.reserve(vars_.size());
  for (auto &v : vars_)
    if (!gone[(size_t)v->id]) {  // (variables are disjoint intervals: a removed start index is one of ms)
      v->id -= before[(size_t)v->id];
      keep.push_back(v);
    }
  vars_ = keep;
  for (const auto &m : ms) m->id = -1;
  N_ = Nn;
}

// algorithmic FP64 FLOPs of one EKFUpdate with r rows over n columns of an N-dim state (SURVEY.md §8(d)
// F_ekf: M = P H^T, S, its factor, K, P - K M^T, dx) and the bytes it must move at least (P read and
// written once, H and the residual read)
double ekf_flops(double N, double n, double r) {
  return 2 * N * n * r + 2 * r * n * n + 2 * r * r * n + r * r * r + 2 * N * r * r + N * N * r + 2 * N * r;
}
double ekf_bytes(double N, double n, double r) { return 8.0 * (2 * N * N + r * (n + 1) + N); }

void Engine::apply_dx(const double *dx) {
  for (auto &v : vars_) v->update(dx + v->id);
  if (o_.do_calib_camera_intrinsics)
    for (auto &c : calib_intr_)
      for (int k = 0; k < 8; k++) cams_[c.first].v[k] = c.second->val[k];
}

// EKF update of P on the device with rows H (r x n, ld) / residual; dx applied to the host mean
void Engine::ekf_update_rows(const double *Hdev, int ldh, int r, int n, const std::vector<int> &hidx,
                             const double *resdev, int res_stride, double sigma2) {
  if (r <= 0) return;
  if (r > kMaxEkfRows) throw HpError(UVIO_HP_E_CAPACITY, "direct EKF update with more than 255 rows");
  const int *hidx_dev = stage(hidx.data(), (size_t)n);
  stage_flush();
  {
    HPROF("ekf_rows.launch");
    KScope ks(&kprof_, KC_EKF);
    launch_ekf_update(d_.stream, d_.P, d_.ldp, N_, Hdev, ldh, r, n, hidx_dev, resdev, res_stride, sigma2, d_.ekf);
    ++p_epoch_;
  }
  kprof_.credit(KC_EKF, ekf_flops(N_, n, r), ekf_bytes(N_, n, r));
  read_dx("EKFUpdate");
  apply_dx(d_.dx_host);
}

// The information-form update's prefactor (launch_ekf_info_pre: P_II = L L^T, V = P[:,I] L^-T) for the
// columns hidx of the state as it is now, on the side stream, behind everything enqueued so far; the
// next information-form update (engine_chain.cpp) on the same columns and state size waits for it instead of factoring again.  Between
// the two calls only kernels that read P may be enqueued (the feature group, chi2 gate and Gram do).
void Engine::info_prefactor(const std::vector<int> &hidx) {
  const int n = (int)hidx.size();
  if (n < 1 || n > d_.max_ncol) return;
  const int slot = d_.pre_slot;
  d_.pre_slot = (d_.pre_slot + 1) % DeviceBufs::kPreSlots;
  int *hh = d_.hidx_pre_h + (size_t)slot * d_.max_ncol, *hd = d_.hidx_pre + (size_t)slot * d_.max_ncol;
  HP_HIP(hipEventSynchronize(d_.ev_pre[slot]));  // this slot's copy, kPreSlots prefactors ago, has run
  std::memcpy(hh, hidx.data(), sizeof(int) * n);
  HP_HIP(hipEventRecord(d_.ev_aux_in, d_.stream));
  HP_HIP(hipStreamWaitEvent(d_.aux, d_.ev_aux_in, 0));
  HP_HIP(hipMemcpyAsync(hd, hh, sizeof(int) * n, hipMemcpyHostToDevice, d_.aux));
  HP_HIP(hipEventRecord(d_.ev_pre[slot], d_.aux));
  launch_ekf_info_pre(d_.aux, d_.P, d_.ldp, N_, n, hd, d_.ekf);
  HP_HIP(hipEventRecord(d_.ev_aux_out, d_.aux));
  d_.pre_hidx = hidx;
  d_.pre_N = N_;
  d_.pre_epoch = p_epoch_;
}

// StateHelper::set_initial_covariance (StateHelper.cpp:199-223).  Start-up only (initialize_with_gt,
// anchor init): P is read back, the blocks are written, and P is re-uploaded.
void Engine::set_initial_covariance(const std::vector<double> &cov, const std::vector<VarP> &order) {
  std::vector<double> Ph;
  download_P(Ph);
  int ii = 0;
  for (auto &a : order) {
    int kk = 0;
    for (auto &b : order) {
      for (int i = 0; i < a->size; i++)
        for (int j = 0; j < b->size; j++) {
          int ncov = 0;
          for (auto &c : order) ncov += c->size;
          Ph[(size_t)(a->id + i) * N_ + b->id + j] = cov[(size_t)(ii + i) * ncov + kk + j];
        }
      kk += b->size;
    }
    ii += a->size;
  }
  for (int i = 0; i < N_; i++)
    for (int j = 0; j < i; j++) Ph[(size_t)i * N_ + j] = Ph[(size_t)j * N_ + i];
  upload_P_full(Ph, N_);
}

// StateHelper::initialize_invertible (StateHelper.cpp:484-577) — start-up only (UWB extrinsic /
// anchor initialization in the UVioManager ctor, UVioManager.cpp:33-55, 221-247).
void Engine::initialize_invertible_host(const VarP &v, const std::vector<std::pair<int, int>> &H_order,
                                        const std::vector<double> &H_R, const std::vector<double> &H_L,
                                        const std::vector<double> &R, const std::vector<double> &res) {
  int r = (int)res.size(), sz = v->size;
  int nh = 0;
  for (auto &h : H_order) nh += h.second;
  std::vector<int> idx;
  for (auto &h : H_order)
    for (int k = 0; k < h.second; k++) idx.push_back(h.first + k);
  std::vector<double> Ph;
  download_P(Ph);
  int N = N_;
  // M_a = P[:, idx] H_R^T (N x r)
  std::vector<double> Ma((size_t)N * r, 0.0);
  for (int i = 0; i < N; i++)
    for (int a = 0; a < r; a++) {
      double s = 0;
      for (int k = 0; k < nh; k++) s += Ph[(size_t)i * N + idx[k]] * H_R[a * nh + k];
      Ma[(size_t)i * r + a] = s;
    }
  // M = H_R P_small H_R^T + R
  std::vector<double> M((size_t)r * r);
  for (int a = 0; a < r; a++)
    for (int b = 0; b < r; b++) {
      double s = 0;
      for (int k = 0; k < nh; k++) s += H_R[a * nh + k] * Ma[(size_t)idx[k] * r + b];
      M[a * r + b] = s + R[a * r + b];
    }
  // H_L^-1 (small, Gauss-Jordan)
  std::vector<double> A = H_L, Inv((size_t)sz * sz, 0.0);
  for (int i = 0; i < sz; i++) Inv[i * sz + i] = 1;
  for (int c = 0; c < sz; c++) {
    int piv = c;
    for (int i = c + 1; i < sz; i++)
      if (std::fabs(A[i * sz + c]) > std::fabs(A[piv * sz + c])) piv = i;
    for (int j = 0; j < sz; j++) std::swap(A[c * sz + j], A[piv * sz + j]), std::swap(Inv[c * sz + j], Inv[piv * sz + j]);
    double d = A[c * sz + c];
    for (int j = 0; j < sz; j++) A[c * sz + j] /= d, Inv[c * sz + j] /= d;
    for (int i = 0; i < sz; i++)
      if (i != c) {
        double f = A[i * sz + c];
        for (int j = 0; j < sz; j++) A[i * sz + j] -= f * A[c * sz + j], Inv[i * sz + j] -= f * Inv[c * sz + j];
      }
  }
  int Nn = N + sz;
  std::vector<double> Pn((size_t)Nn * Nn, 0.0);
  for (int i = 0; i < N; i++) std::memcpy(&Pn[(size_t)i * Nn], &Ph[(size_t)i * N], sizeof(double) * N);
  for (int i = 0; i < N; i++)
    for (int a = 0; a < sz; a++) {
      double s = 0;
      for (int b = 0; b < r; b++) s += Ma[(size_t)i * r + b] * Inv[a * sz + b];
      Pn[(size_t)i * Nn + N + a] = -s;
      Pn[(size_t)(N + a) * Nn + i] = -s;
    }
  for (int a = 0; a < sz; a++)
    for (int b = 0; b < sz; b++) {
      double s = 0;
      for (int c = 0; c < r; c++)
        for (int e = 0; e < r; e++) s += Inv[a * sz + c] * M[c * r + e] * Inv[b * sz + e];
      Pn[(size_t)(N + a) * Nn + N + b] = s;
    }
  std::vector<double> dxv(sz, 0.0);
  for (int a = 0; a < sz; a++)
    for (int b = 0; b < r; b++) dxv[a] += Inv[a * sz + b] * res[b];
  v->update(dxv.data());
  v->id = N;
  vars_.push_back(v);
  N_ = Nn;
  upload_P_full(Pn, Nn);
}

int Engine::state_vector(double *out, int cap, int *meta, int meta_cap, int *nvars, bool fej) {
  int k = 0, nv = 0;
  for (auto &v : vars_) {
    if (meta && 3 * nv + 2 < meta_cap) {
      meta[3 * nv] = v->kind;
      meta[3 * nv + 1] = v->id;
      meta[3 * nv + 2] = v->size;
    }
    for (int i = 0; i < v->vlen; i++) {
      if (k < cap) out[k] = fej ? v->fej[i] : v->val[i];
      k++;
    }
    nv++;
  }
  if (nvars) *nvars = nv;
  return k;
}

std::vector<double> Engine::clone_times() const {
  std::vector<double> t;
  for (auto &c : clones_) t.push_back(c.first);
  return t;
}

}  // namespace uvhp

namespace uvhp {

// Standalone StateHelper::EKFUpdate on a caller-provided covariance (kernel-level parity entry):
// the same device kernels the manager uses, on temporary device buffers.
int Engine::ekf_update_standalone(double *P, int N, const int *H_index, int n, const double *H, int r,
                                  const double *res, double sigma2, double *dx_out, bool compress) {
  if (!P || N <= 0 || n <= 0 || r <= 0 || !H || !res || !H_index || !dx_out) return UVIO_HP_E_ARG;
  for (int j = 0; j < n; j++)
    if (H_index[j] < 0 || H_index[j] >= N) return UVIO_HP_E_ARG;
  // the limits the launchers would throw on, checked before anything is created: the factor panels hold 256 rows
  // (the direct form's r rows and the information form's n columns, each with its augmented row), and k_ekf_MS
  // stages 16 rows of P[:, I] in LDS
  bool info = compress && r > n;
  if (info ? n > kMaxEkfRows : r > kMaxEkfRows) return UVIO_HP_E_CAPACITY;
  if (!info && (size_t)16 * (n | 1) * sizeof(double) > (size_t)kMaxDynLds) return UVIO_HP_E_CAPACITY;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return UVIO_HP_E_DEVICE;
  Stream s = Stream::create();
  int ldh = n + 1;
  int rw = std::max(r, n + 1);
  int nch = gram_num_chunks(r);
  DevBuf<double> dP((size_t)N * N), dH((size_t)r * ldh);
  // M and W also serve as the (n + 1) x (n | 1) work matrices of the split information-form factors
  // (launch_ekf_info_pre / _post), one row more than N when every state is measured (N == n)
  const size_t mw = (size_t)std::max(N, n + 1) * rw;
  DevBuf<double> dM(mw), dW(mw), dS((size_t)5 * rw * rw), dy(rw), dDinv((size_t)(rw / 16 + 1) * 256), dPart, dG;
  if (info) {
    dPart = DevBuf<double>((size_t)nch * ldh * ldh);
    dG = DevBuf<double>((size_t)ldh * ldh);
  }
  DevBuf<double> ddx(N);
  DevBuf<int> dI(n), dneg(2 + n);
  std::vector<double> Ha((size_t)r * ldh);
  for (int i = 0; i < r; i++) {
    std::memcpy(&Ha[(size_t)i * ldh], H + (size_t)i * n, sizeof(double) * n);
    Ha[(size_t)i * ldh + n] = res[i];
  }
  HP_HIP(hipMemcpyAsync(dP, P, sizeof(double) * N * N, hipMemcpyHostToDevice, s));
  HP_HIP(hipMemcpyAsync(dH, Ha.data(), sizeof(double) * Ha.size(), hipMemcpyHostToDevice, s));
  HP_HIP(hipMemcpyAsync(dI, H_index, sizeof(int) * n, hipMemcpyHostToDevice, s));
  HP_HIP(hipMemsetAsync(dneg, 0, sizeof(int), s));
  EkfScratch sc{dM, dW, dS, dy, ddx, dneg, dDinv};
  if (info) {
    int nc2 = 0;
    launch_gram(s, dH, r, ldh, ldh, dPart, &nc2);
    launch_ekf_info(s, dP, N, N, dPart, nc2, n, dI, sigma2, dG, sc);
  } else {
    launch_ekf_update(s, dP, N, N, dH, ldh, r, n, dI, dH + n, ldh, sigma2, sc);
  }
  int neg = 0;
  HP_HIP(hipMemcpyAsync(P, dP, sizeof(double) * N * N, hipMemcpyDeviceToHost, s));
  HP_HIP(hipMemcpyAsync(dx_out, ddx, sizeof(double) * N, hipMemcpyDeviceToHost, s));
  HP_HIP(hipMemcpyAsync(&neg, dneg, sizeof(int), hipMemcpyDeviceToHost, s));
  HP_HIP(hipStreamSynchronize(s));  // nothing in flight when the buffers go (on a throw: freeing device memory waits by itself)
  return neg > 0 ? UVIO_HP_E_NUMERIC : 0;
}

// H (r x n, ld ldh), res (r) and the upper triangle of R (r x r, ld ldr) hold finite numbers only
bool ekf_R_inputs_finite(const double *H, int ldh, int r, int n, const double *res, const double *R, int ldr) {
  for (int i = 0; i < r; i++) {
    for (int j = 0; j < n; j++)
      if (!std::isfinite(H[(size_t)i * ldh + j])) return false;
    if (!std::isfinite(res[i])) return false;
    for (int j = i; j < r; j++)
      if (!std::isfinite(R[(size_t)i * ldr + j])) return false;
  }
  return true;
}

// ekf_update_standalone's direct form with the caller's dense R (upper triangle) and the chi2 gate on the update's
// own factor (launch_ekf_update_R): the same buffers and checks.  Not applied (gated, or S not positive definite:
// UVIO_HP_E_ARG): P is not written and dx_out is zeros.
int Engine::ekf_update_R_standalone(double *P, int N, const int *H_index, int n, const double *H, int r,
                                    const double *res, const double *R, int ldr, double chi2_thr, double *dx_out,
                                    double *chi2, int *applied) {
  if (!P || N <= 0 || n <= 0 || r <= 0 || !H || !res || !H_index || !dx_out || !R || !chi2 || !applied)
    return UVIO_HP_E_ARG;
  if (ldr < r || !(chi2_thr > 0.0)) return UVIO_HP_E_ARG;
  for (int j = 0; j < n; j++)
    if (H_index[j] < 0 || H_index[j] >= N) return UVIO_HP_E_ARG;
  if (r > kMaxEkfRows) return UVIO_HP_E_CAPACITY;
  if ((size_t)16 * (n | 1) * sizeof(double) > (size_t)kMaxDynLds) return UVIO_HP_E_CAPACITY;
  if (!ekf_R_inputs_finite(H, n, r, n, res, R, ldr)) return UVIO_HP_E_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return UVIO_HP_E_DEVICE;
  Stream s = Stream::create();
  const int ldh = n + 1;
  DevBuf<double> dP((size_t)N * N), dH((size_t)r * ldh), dR((size_t)r * r);
  DevBuf<double> dM((size_t)N * r), dW((size_t)N * r), dS((size_t)5 * r * r), dy(r), dDinv((size_t)(r / 16 + 1) * 256);
  DevBuf<double> ddx((size_t)N + 2);  // [dx | chi2, accepted]
  DevBuf<int> dI(n), dneg(2);         // [negative diagonals, gate]
  std::vector<double> Ha((size_t)r * ldh), Ru((size_t)r * r, 0.0);
  for (int i = 0; i < r; i++) {
    std::memcpy(&Ha[(size_t)i * ldh], H + (size_t)i * n, sizeof(double) * n);
    Ha[(size_t)i * ldh + n] = res[i];
    for (int j = i; j < r; j++) Ru[(size_t)i * r + j] = R[(size_t)i * ldr + j];
  }
  HP_HIP(hipMemcpyAsync(dP, P, sizeof(double) * N * N, hipMemcpyHostToDevice, s));
  HP_HIP(hipMemcpyAsync(dH, Ha.data(), sizeof(double) * Ha.size(), hipMemcpyHostToDevice, s));
  HP_HIP(hipMemcpyAsync(dR, Ru.data(), sizeof(double) * Ru.size(), hipMemcpyHostToDevice, s));
  HP_HIP(hipMemcpyAsync(dI, H_index, sizeof(int) * n, hipMemcpyHostToDevice, s));
  HP_HIP(hipMemsetAsync(dneg, 0, 2 * sizeof(int), s));
  EkfScratch sc{dM, dW, dS, dy, ddx, dneg, dDinv};
  sc.chi2_gate = dneg + 1;
  launch_ekf_update_R(s, dP, N, N, dH, ldh, r, n, dI, dH + n, ldh, dR, r, chi2_thr, sc);
  int neg = 0;
  double g[2] = {0.0, 0.0};
  HP_HIP(hipMemcpyAsync(g, ddx + N, sizeof(g), hipMemcpyDeviceToHost, s));
  HP_HIP(hipMemcpyAsync(&neg, dneg, sizeof(int), hipMemcpyDeviceToHost, s));
  HP_HIP(hipStreamSynchronize(s));
  *chi2 = g[0];
  *applied = g[1] != 0.0 ? 1 : 0;
  if (!*applied) {
    std::fill(dx_out, dx_out + N, 0.0);
    if (!std::isfinite(g[0]))
      throw HpError(UVIO_HP_E_ARG, "ekf_update_R: S = H P H^T + R is not positive definite; nothing was applied");
    return 0;
  }
  HP_HIP(hipMemcpyAsync(P, dP, sizeof(double) * N * N, hipMemcpyDeviceToHost, s));
  HP_HIP(hipMemcpyAsync(dx_out, ddx, sizeof(double) * N, hipMemcpyDeviceToHost, s));
  HP_HIP(hipStreamSynchronize(s));  // nothing in flight when the buffers go
  return neg > 0 ? UVIO_HP_E_NUMERIC : 0;
}

// Standalone measurement compression: R factor of [H | res] (m x (n+1)) via the Gram + Cholesky kernels
int Engine::compress_standalone(const double *A, int m, int n, double *R_out) {
  if (!A || m <= 0 || n <= 0 || !R_out) return UVIO_HP_E_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return UVIO_HP_E_DEVICE;
  Stream s = Stream::create();
  int ncol = n + 1;
  int nch = gram_num_chunks(m);
  DevBuf<double> dA((size_t)m * ncol), dPart((size_t)nch * ncol * ncol), dR((size_t)2 * ncol * ncol);
  HP_HIP(hipMemcpyAsync(dA, A, sizeof(double) * m * ncol, hipMemcpyHostToDevice, s));
  int nc2 = 0;
  launch_gram(s, dA, m, ncol, ncol, dPart, &nc2);
  launch_gram_reduce_chol(s, dPart, nc2, ncol, dR, ncol);
  HP_HIP(hipMemcpyAsync(R_out, dR, sizeof(double) * ncol * ncol, hipMemcpyDeviceToHost, s));
  HP_HIP(hipStreamSynchronize(s));  // nothing in flight when the buffers go (on a throw: freeing device memory waits by itself)
  return 0;
}

// CamBase::undistort_f (ov_core/src/cam/CamBase.h:89, CamRadtan.h:99 / CamEqui.h:108) over n points on the
// device; the points whose float result could depend on the equidistant model's tan (cam_undistort_f's flag)
// are recomputed here with the host's libm, so uvn is the host's result for every point.
int Engine::undistort_standalone(int model, const double cam[8], int n, const float *uv, float *uvn, uint8_t *amb) {
  if ((model != 0 && model != 1) || !cam || n < 0 || (n > 0 && (!uv || !uvn))) return UVIO_HP_E_ARG;
  if (n == 0) return 0;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return UVIO_HP_E_DEVICE;
  CamParams c{};
  c.model = model;
  for (int k = 0; k < 8; k++) c.v[k] = cam[k];
  Stream s = Stream::create();
  DevBuf<float> d_uv(2 * (size_t)n), d_uvn(2 * (size_t)n);
  DevBuf<uint8_t> d_amb(n);
  std::vector<uint8_t> h_amb(n);
  HP_HIP(hipMemcpyAsync(d_uv, uv, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, s));
  launch_undistort_points(s, c, n, d_uv, d_uvn, d_amb);
  HP_HIP(hipMemcpyAsync(uvn, d_uvn, sizeof(float) * 2 * (size_t)n, hipMemcpyDeviceToHost, s));
  HP_HIP(hipMemcpyAsync(h_amb.data(), d_amb, (size_t)n, hipMemcpyDeviceToHost, s));
  HP_HIP(hipStreamSynchronize(s));  // nothing in flight when the buffers go (on a throw: freeing device memory waits by itself)
  for (int i = 0; i < n; i++) {
    if (h_amb[i]) cam_undistort_f(c, uv[2 * i], uv[2 * i + 1], uvn[2 * i], uvn[2 * i + 1]);
    if (amb) amb[i] = h_amb[i];
  }
  return 0;
}

int Engine::grid_order_standalone(const uint8_t *resp, const int *off, int ncell, int kmax, int depth,
                                  int *arrangement, int *top) {
  if (ncell < 0 || !off || kmax < 0 || kmax > 64 || (kmax > 0 && !top)) return UVIO_HP_E_ARG;
  if (depth > kSortStack) return UVIO_HP_E_ARG;  // every level of the depth limit may leave a segment on the stack
  if (ncell == 0) return 0;
  int nmax = 0;
  for (int c = 0; c < ncell; c++) {
    if (off[c + 1] < off[c]) return UVIO_HP_E_ARG;
    nmax = std::max(nmax, off[c + 1] - off[c]);
  }
  const int total = off[ncell];
  if (total > 0 && (!resp || !arrangement)) return UVIO_HP_E_ARG;
  if (nmax > 16384) return UVIO_HP_E_CAPACITY;  // 8 bytes of LDS per candidate
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return UVIO_HP_E_DEVICE;
  Stream s = Stream::create();
  const size_t ntop = (size_t)ncell * (size_t)std::max(kmax, 1);
  DevBuf<uint8_t> d_resp(total);
  DevBuf<int> d_off((size_t)ncell + 1), d_arr(total), d_top(ntop);
  if (total > 0) HP_HIP(hipMemcpyAsync(d_resp, resp, (size_t)total, hipMemcpyHostToDevice, s));
  HP_HIP(hipMemcpyAsync(d_off, off, sizeof(int) * (size_t)(ncell + 1), hipMemcpyHostToDevice, s));
  if (kmax > 0) HP_HIP(hipMemcpyAsync(d_top, top, sizeof(int) * ntop, hipMemcpyHostToDevice, s));
  launch_grid_order_probe(s, d_resp, d_off, ncell, nmax, kmax, depth, d_arr, d_top);
  HP_HIP(hipGetLastError());
  if (total > 0) HP_HIP(hipMemcpyAsync(arrangement, d_arr, sizeof(int) * (size_t)total, hipMemcpyDeviceToHost, s));
  if (kmax > 0) HP_HIP(hipMemcpyAsync(top, d_top, sizeof(int) * ntop, hipMemcpyDeviceToHost, s));
  HP_HIP(hipStreamSynchronize(s));  // nothing in flight when the buffers go (on a throw: freeing device memory waits by itself)
  return 0;
}

// histogram_method 2 on a caller-given image: the tracker's own launch_pyramids on a one-level pyramid
int Engine::clahe_standalone(const uint8_t *img, int w, int h, int stride, uint8_t *out) {
  if (!img || !out || w <= kClaheTiles || h <= kClaheTiles || stride < w) return UVIO_HP_E_ARG;
  if (w > 16384 || h > 16384) return UVIO_HP_E_CAPACITY;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return UVIO_HP_E_DEVICE;
  const size_t n = (size_t)w * h;
  Stream s = Stream::create();
  DevBuf<uint8_t> d_src(n), d_img(n), d_lut(kClaheLutBytes);
  DevBuf<int16_t> d_der(2 * n);
  PyrJob job{};
  job.ncam = 1;
  job.method = 2;
  job.p[0].levels = 1;
  job.p[0].w[0] = w;
  job.p[0].h[0] = h;
  job.p[0].img[0] = d_img;
  job.p[0].der[0] = d_der;
  job.src[0] = d_src;
  job.stride[0] = w;
  job.clahe[0] = d_lut;
  HP_HIP(hipMemcpy2DAsync(d_src, w, img, stride, w, h, hipMemcpyHostToDevice, s));
  launch_pyramids(s, job);
  HP_HIP(hipGetLastError());
  HP_HIP(hipMemcpyAsync(out, d_img, n, hipMemcpyDeviceToHost, s));
  HP_HIP(hipStreamSynchronize(s));  // nothing in flight when the buffers go (on a throw: freeing device memory waits by itself)
  return 0;
}

// ---- caller-defined state variables: host helpers, the random walk, the standalone twins ----
bool aux_upper_ok(const double *A, int ld, int d, bool pos_diag) {
  for (int i = 0; i < d; i++) {
    for (int j = i; j < d; j++)
      if (!std::isfinite(A[(size_t)i * ld + j])) return false;
    if (pos_diag && !(A[(size_t)i * ld + i] > 0.0)) return false;
  }
  return true;
}

bool aux_inverse(const double *A0, int lda, int d, double *inv) {
  double A[UVIO_HP_AUX_MAX_DIM * UVIO_HP_AUX_MAX_DIM], amax = 0.0;
  for (int i = 0; i < d; i++)
    for (int j = 0; j < d; j++) {
      const double v = A0[(size_t)i * lda + j];
      if (!std::isfinite(v)) return false;
      A[i * d + j] = v;
      amax = std::max(amax, std::fabs(v));
      inv[i * d + j] = i == j ? 1.0 : 0.0;
    }
  const double tiny = d * 2.220446049250313e-16 * amax;
  for (int c = 0; c < d; c++) {
    int piv = c;
    for (int i = c + 1; i < d; i++)
      if (std::fabs(A[i * d + c]) > std::fabs(A[piv * d + c])) piv = i;
    if (!(std::fabs(A[piv * d + c]) > tiny)) return false;
    for (int j = 0; j < d; j++) std::swap(A[c * d + j], A[piv * d + j]), std::swap(inv[c * d + j], inv[piv * d + j]);
    const double p = A[c * d + c];
    for (int j = 0; j < d; j++) A[c * d + j] /= p, inv[c * d + j] /= p;
    for (int i = 0; i < d; i++)
      if (i != c) {
        const double f = A[i * d + c];
        for (int j = 0; j < d; j++) A[i * d + j] -= f * A[c * d + j], inv[i * d + j] -= f * inv[c * d + j];
      }
  }
  for (int k = 0; k < d * d; k++)
    if (!std::isfinite(inv[k])) return false;
  return true;
}

void Engine::aux_walk(double dt) {
  if (aux_walkers_ == 0) return;
  int m = 0;
  for (const auto &a : aux_)
    if (a.second.walks) m += a.second.v->size;
  void *hv = nullptr;
  char *dv = (char *)stage_reserve(sizeof(double) * m + sizeof(int) * m, &hv);
  double *hs = (double *)hv;
  int *hi = (int *)(hs + m);
  int j = 0;
  for (const auto &a : aux_)
    if (a.second.walks)
      for (int k = 0; k < a.second.v->size; k++, j++) hs[j] = a.second.s2[k], hi[j] = a.second.v->id + k;
  stage_flush();
  launch_aux_walk(d_.stream, d_.P, d_.ldp, (const int *)(dv + sizeof(double) * m), (const double *)dv, m, dt);
  ++p_epoch_;
}

// the shared front of the twins: the covariance rows with their padding go up, one kernel group runs at the caller's
// leading dimension, the rows come back
template <class Fn>
static int aux_standalone_run(double *P, size_t rows, int ld, Fn &&run) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return UVIO_HP_E_DEVICE;
  Stream s = Stream::create();
  DevBuf<double> dP(rows * (size_t)ld);
  HP_HIP(hipMemcpyAsync(dP, P, sizeof(double) * rows * ld, hipMemcpyHostToDevice, s));
  run((hipStream_t)s, (double *)dP);
  HP_HIP(hipGetLastError());
  HP_HIP(hipMemcpyAsync(P, dP, sizeof(double) * rows * ld, hipMemcpyDeviceToHost, s));
  HP_HIP(hipStreamSynchronize(s));  // nothing in flight when the buffers go
  return 0;
}

int Engine::aux_append_standalone(double *P, int N, int ld, int dim, const double *prior, int ldp) {
  if (!P || !prior || N < 0 || dim < 1 || dim > UVIO_HP_AUX_MAX_DIM || ldp < dim) return UVIO_HP_E_ARG;
  if ((long long)N + dim > ld) return UVIO_HP_E_ARG;
  if (!aux_upper_ok(prior, ldp, dim, true)) return UVIO_HP_E_ARG;
  std::vector<double> pr((size_t)dim * dim, 0.0);
  for (int i = 0; i < dim; i++)
    for (int j = i; j < dim; j++) pr[(size_t)i * dim + j] = prior[(size_t)i * ldp + j];
  DevBuf<double> dpr;
  return aux_standalone_run(P, (size_t)N + dim, ld, [&](hipStream_t s, double *dP) {
    dpr = DevBuf<double>(pr.size());
    HP_HIP(hipMemcpyAsync(dpr, pr.data(), sizeof(double) * pr.size(), hipMemcpyHostToDevice, s));
    launch_aux_append(s, dP, ld, N, dim, dpr);
  });
}

int Engine::aux_init_standalone(double *P, int N, int ld, int dim, const int *H_index, int n, const double *H_x,
                                int ldhx, const double *H_auxinv, const double *R, int ldr) {
  if (!P || !H_auxinv || !R || N < 0 || n < 0 || dim < 1 || dim > UVIO_HP_AUX_MAX_DIM || ldr < dim)
    return UVIO_HP_E_ARG;
  if (n > 0 && (!H_index || !H_x || ldhx < n)) return UVIO_HP_E_ARG;
  if ((long long)N + dim > ld) return UVIO_HP_E_ARG;
  if (n > kAuxMaxCols) return UVIO_HP_E_CAPACITY;
  for (int j = 0; j < n; j++)
    if (H_index[j] < 0 || H_index[j] >= N) return UVIO_HP_E_ARG;
  if (!aux_upper_ok(R, ldr, dim, false)) return UVIO_HP_E_ARG;
  // [Hx (dim x n) | Hinv | R upper] as one table
  const size_t nH = (size_t)dim * n, nD = (size_t)dim * dim;
  std::vector<double> tab(nH + 2 * nD, 0.0);
  for (int i = 0; i < dim; i++) {
    for (int k = 0; k < n; k++)
      if (!std::isfinite(tab[(size_t)i * n + k] = H_x[(size_t)i * ldhx + k])) return UVIO_HP_E_ARG;
    for (int j = 0; j < dim; j++) {
      if (!std::isfinite(tab[nH + (size_t)i * dim + j] = H_auxinv[(size_t)i * dim + j])) return UVIO_HP_E_ARG;
      if (j >= i) tab[nH + nD + (size_t)i * dim + j] = R[(size_t)i * ldr + j];
    }
  }
  DevBuf<double> dtab, dMa;
  DevBuf<int> dI;
  return aux_standalone_run(P, (size_t)N + dim, ld, [&](hipStream_t s, double *dP) {
    dtab = DevBuf<double>(tab.size());
    dMa = DevBuf<double>((size_t)std::max(N, 1) * dim);
    dI = DevBuf<int>((size_t)std::max(n, 1));
    HP_HIP(hipMemcpyAsync(dtab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, s));
    if (n > 0) HP_HIP(hipMemcpyAsync(dI, H_index, sizeof(int) * n, hipMemcpyHostToDevice, s));
    launch_aux_init(s, dP, ld, N, dim, dtab, n, n, dI, dtab + nH, dtab + nH + nD, dMa);
  });
}

int Engine::aux_walk_standalone(double *P, int N, int ld, int ntab, const int *ids, const int *dims,
                                const double *sigma2, double dt) {
  if (!P || N < 1 || ld < N || ntab < 0 || !std::isfinite(dt) || dt < 0.0) return UVIO_HP_E_ARG;
  if (ntab > 0 && (!ids || !dims || !sigma2)) return UVIO_HP_E_ARG;
  std::vector<int> cidx;
  std::vector<uint8_t> seen((size_t)N, 0);
  for (int t = 0; t < ntab; t++) {
    if (dims[t] < 1 || dims[t] > UVIO_HP_AUX_MAX_DIM || ids[t] < 0 || (long long)ids[t] + dims[t] > N)
      return UVIO_HP_E_ARG;
    for (int k = 0; k < dims[t]; k++) {
      if (seen[(size_t)(ids[t] + k)]++) return UVIO_HP_E_ARG;  // (the blocks are disjoint)
      cidx.push_back(ids[t] + k);
    }
  }
  const int m = (int)cidx.size();
  for (int j = 0; j < m; j++)
    if (!std::isfinite(sigma2[j]) || sigma2[j] < 0.0) return UVIO_HP_E_ARG;
  DevBuf<double> ds2;
  DevBuf<int> dI;
  return aux_standalone_run(P, (size_t)N, ld, [&](hipStream_t s, double *dP) {
    if (m == 0) return;
    ds2 = DevBuf<double>((size_t)m);
    dI = DevBuf<int>((size_t)m);
    HP_HIP(hipMemcpyAsync(ds2, sigma2, sizeof(double) * m, hipMemcpyHostToDevice, s));
    HP_HIP(hipMemcpyAsync(dI, cidx.data(), sizeof(int) * m, hipMemcpyHostToDevice, s));
    launch_aux_walk(s, dP, ld, dI, ds2, m, dt);
  });
}

// n indices, each in [0, N); distinct when asked
static bool cov_indices_ok(const int *v, int n, int N, bool distinct) {
  std::vector<uint8_t> seen((size_t)std::max(N, 0), 0);
  for (int k = 0; k < n; k++) {
    if (v[k] < 0 || v[k] >= N) return false;
    if (distinct && seen[(size_t)v[k]]++) return false;
  }
  return true;
}

// Engine::cov_propagate / cov_propagate_clone + clone_imu_pose's launches on a caller's covariance
int Engine::cov_propagate_standalone(double *P, int N, int ld, int s0, int p, const int *rows, const int *iold, int q,
                                     const double *Phi, const double *Q, int clone, int src0, int dt_id,
                                     const double *dnc, int path, int *path_ran) {
  if (!P || !iold || !Phi || !Q || !path_ran) return UVIO_HP_E_ARG;
  const bool do_clone = clone != 0, do_dt = do_clone && dt_id >= 0;
  if (N < 1 || p < 1 || q < 1 || (long long)N + (do_clone ? 6 : 0) > ld) return UVIO_HP_E_ARG;
  if (path != UVIO_HP_COV_PATH_AUTO && path != UVIO_HP_COV_PATH_SPLIT && path != UVIO_HP_COV_PATH_FUSED)
    return UVIO_HP_E_ARG;
  if ((rows && do_clone) || (path == UVIO_HP_COV_PATH_FUSED && !do_clone) || (do_dt && !dnc)) return UVIO_HP_E_ARG;
  if (p > 64 || q > 256) return UVIO_HP_E_CAPACITY;  // (Engine::cov_propagate's limits)
  if (rows ? !cov_indices_ok(rows, p, N, true) : (s0 < 0 || (long long)s0 + p > N)) return UVIO_HP_E_ARG;
  if (!cov_indices_ok(iold, q, N, true)) return UVIO_HP_E_ARG;
  if (do_clone && (src0 < 0 || (long long)src0 + 6 > N || dt_id >= N)) return UVIO_HP_E_ARG;
  const bool fits = do_clone && prop_clone_fits(N, p, q);
  if (path == UVIO_HP_COV_PATH_FUSED && !fits) return UVIO_HP_E_CAPACITY;
  const bool fused = fits && path != UVIO_HP_COV_PATH_SPLIT;
  // [Phi | Q | dnc] as one table
  const size_t nPhi = (size_t)p * q, nQ = (size_t)p * p;
  std::vector<double> tab(nPhi + nQ + 6, 0.0);
  std::copy(Phi, Phi + nPhi, tab.begin());
  std::copy(Q, Q + nQ, tab.begin() + (ptrdiff_t)nPhi);
  if (do_dt) std::copy(dnc, dnc + 6, tab.begin() + (ptrdiff_t)(nPhi + nQ));
  std::vector<int> itab(iold, iold + q);
  if (rows) itab.insert(itab.end(), rows, rows + p);
  DevBuf<double> dtab, dT;
  DevBuf<int> dI;
  const int rc = aux_standalone_run(P, (size_t)N + (do_clone ? 6 : 0), ld, [&](hipStream_t s, double *dP) {
    dtab = DevBuf<double>(tab.size());
    dT = DevBuf<double>((size_t)N * p);
    dI = DevBuf<int>(itab.size());
    HP_HIP(hipMemcpyAsync(dtab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, s));
    HP_HIP(hipMemcpyAsync(dI, itab.data(), sizeof(int) * itab.size(), hipMemcpyHostToDevice, s));
    const double *dPhi = dtab, *dQ = dtab + nPhi, *ddnc = dtab + nPhi + nQ;
    const int did = do_dt ? dt_id : 0;
    if (fused) {
      if (!launch_prop_clone(s, dP, ld, N, s0, p, dI, q, dPhi, dQ, dT, src0, did, ddnc, do_dt ? 1 : 0))
        throw HpError(UVIO_HP_E_CAPACITY, "fused propagation refused after the size check");
      return;
    }
    launch_cov_propagate(s, dP, ld, N, s0, p, dI, q, dPhi, dQ, dT, rows ? dI + q : nullptr);
    if (do_clone) launch_clone(s, dP, ld, N, src0, did, ddnc, do_dt ? 1 : 0);
  });
  if (rc) return rc;
  *path_ran = fused ? UVIO_HP_COV_PATH_FUSED : UVIO_HP_COV_PATH_SPLIT;
  return 0;
}

// Engine::marginalize / marginalize_many / marginalize_slots / the marginal-covariance gather's launch on a caller's
// covariance, into a caller's output
int Engine::cov_gather_standalone(const double *P, int N, int ld, int op, int m0, int ms, const int *idx, int n,
                                  double *out) {
  if (!P || !out || N < 1 || ld < N) return UVIO_HP_E_ARG;
  int Nn = 0;
  if (op == UVIO_HP_COV_MARGINALIZE) {
    if (m0 < 0 || ms < 1 || (long long)m0 + ms > N) return UVIO_HP_E_ARG;
    Nn = N - ms;
  } else if (op == UVIO_HP_COV_MARGINALIZE_MULTI || op == UVIO_HP_COV_COMPACT || op == UVIO_HP_COV_MARGINAL_GATHER) {
    if (n < 0 || (n > 0 && !idx)) return UVIO_HP_E_ARG;
    if (op == UVIO_HP_COV_MARGINAL_GATHER ? n > 4096 : n > N)
      return op == UVIO_HP_COV_MARGINAL_GATHER ? UVIO_HP_E_CAPACITY : UVIO_HP_E_ARG;
    if (!cov_indices_ok(idx, n, N, false)) return UVIO_HP_E_ARG;
    if (op == UVIO_HP_COV_MARGINALIZE_MULTI)
      for (int k = 1; k < n; k++)
        if (idx[k] <= idx[k - 1]) return UVIO_HP_E_ARG;  // (the kept indices, in the covariance's order)
    Nn = n;
  } else {
    return UVIO_HP_E_ARG;
  }
  if (Nn == 0) return 0;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return UVIO_HP_E_DEVICE;
  const bool dense = op == UVIO_HP_COV_MARGINAL_GATHER;
  const size_t nout = (size_t)Nn * (dense ? (size_t)Nn : (size_t)ld);
  Stream s = Stream::create();
  DevBuf<double> dP((size_t)N * ld), dout(nout);
  DevBuf<int> dI((size_t)std::max(n, 1));
  HP_HIP(hipMemcpyAsync(dP, P, sizeof(double) * (size_t)N * ld, hipMemcpyHostToDevice, s));
  HP_HIP(hipMemcpyAsync(dout, out, sizeof(double) * nout, hipMemcpyHostToDevice, s));
  if (op != UVIO_HP_COV_MARGINALIZE) HP_HIP(hipMemcpyAsync(dI, idx, sizeof(int) * n, hipMemcpyHostToDevice, s));
  if (op == UVIO_HP_COV_MARGINALIZE)
    launch_marginalize(s, dP, dout, ld, N, m0, ms);
  else if (op == UVIO_HP_COV_MARGINALIZE_MULTI)
    launch_marginalize_multi(s, dP, dout, ld, Nn, dI);
  else if (op == UVIO_HP_COV_COMPACT)
    launch_compact(s, dP, dout, ld, Nn, dI);
  else
    launch_marginal_gather(s, dP, ld, dI, Nn, dout);
  HP_HIP(hipGetLastError());
  HP_HIP(hipMemcpyAsync(out, dout, sizeof(double) * nout, hipMemcpyDeviceToHost, s));
  HP_HIP(hipStreamSynchronize(s));  // nothing in flight when the buffers go
  return 0;
}

// One position fix through k_fix_rows -> k_chain_M -> k_chain_update (Engine::fix_update_chain's launches for a chain
// of one) on a caller's covariance at a caller's pose
int Engine::position_update_standalone(double *P, int N, int ld, int imu_id, const double *q, const double *p,
                                       int aux_id, const double *s, int r, const double *C, const double *z,
                                       const double *R, int ldr, double chi2_thr, double *dx, double *chi2,
                                       int *applied) {
  if (!P || !q || !p || !s || !C || !z || !R || !dx || !chi2 || !applied) return UVIO_HP_E_ARG;
  if (r < 1 || r > 3 || ldr < r || N < 6 || ld < N || !(chi2_thr > 0.0)) return UVIO_HP_E_ARG;
  if (imu_id < 0 || (long long)imu_id + 6 > N) return UVIO_HP_E_ARG;
  if (aux_id >= 0 && ((long long)aux_id + 3 > N || (aux_id + 3 > imu_id && aux_id < imu_id + 6))) return UVIO_HP_E_ARG;
  if (!aux_upper_ok(R, ldr, r, true)) return UVIO_HP_E_ARG;
  DFixState st{};
  bool finite = true;
  for (int k = 0; k < 4; k++) finite = finite && std::isfinite(st.q[k] = q[k]);
  for (int k = 0; k < 3; k++) finite = finite && std::isfinite(st.p[k] = p[k]) && std::isfinite(st.s[0][k] = s[k]);
  for (int i = 0; i < r; i++) {
    for (int k = 0; k < 3; k++) finite = finite && std::isfinite(st.C[0][3 * i + k] = C[3 * i + k]);
    finite = finite && std::isfinite(st.z[0][i] = z[i]);
    for (int j = i; j < r; j++) st.R[0][3 * i + j] = st.R[0][3 * j + i] = R[(size_t)i * ldr + j];
  }
  if (!finite) return UVIO_HP_E_ARG;
  st.thr[0] = chi2_thr;
  st.r[0] = r;
  st.id_aux[0] = aux_id >= 0 ? aux_id : -1;
  st.id_imu = imu_id;
  st.nf = 1;
  DevBuf<DFixState> dst;
  DevBuf<DChainRow> drow;
  DevBuf<double> dM;
  DevBuf<unsigned char> dreg;
  std::vector<double> reg((size_t)N + kChainHeader, 0.0);
  const int rc = aux_standalone_run(P, (size_t)N, ld, [&](hipStream_t sm, double *dP) {
    dst = DevBuf<DFixState>(1);
    drow = DevBuf<DChainRow>(1);
    dM = DevBuf<double>((size_t)3 * N);
    dreg = DevBuf<unsigned char>(sizeof(double) * reg.size());
    DChainRegion *region = chain_region(dreg, reg.size(), 0);
    HP_HIP(hipMemcpyAsync(dst, &st, sizeof(st), hipMemcpyHostToDevice, sm));
    HP_HIP(hipMemsetAsync(dreg, 0, sizeof(double) * reg.size(), sm));
    launch_fix_rows(sm, dst, 0, nullptr, drow, region);
    launch_chain_M(sm, dP, ld, N, drow, r, dM);
    launch_chain_update(sm, dP, ld, N, dM, drow, r, false, region);
    HP_HIP(hipMemcpyAsync(reg.data(), dreg, sizeof(double) * reg.size(), hipMemcpyDeviceToHost, sm));
  });
  if (rc) return rc;
  const DChainRegion g = chain_header(reg.data());
  *chi2 = g.chi2;
  *applied = g.accepted != 0.0 ? 1 : 0;
  for (int i = 0; i < N; i++) dx[i] = *applied ? reg[kChainHeader + i] : 0.0;
  if (g.extra != 0.0) return UVIO_HP_E_ARG;  // refused: S is not positive definite, nothing was applied
  if (*applied && g.neg > 0) return UVIO_HP_E_NUMERIC;
  return 0;
}

// One pose fix through k_pose_rows -> k_chain_M -> k_chain_update (Engine::pose_update_chain's launches for a chain of
// one) on a caller's covariance at a caller's pose, lever arm and mounting rotation
int Engine::pose_update_standalone(double *P, int N, int ld, int imu_id, const double *q, const double *p, int arm_id,
                                   const double *s, int rot_id, const double *q_ItoS, int mode, const double *z_q,
                                   const double *z_p, const double *R, int ldr, double chi2_thr, double *dx,
                                   double *chi2, int *applied) {
  if (!P || !q || !p || !s || !q_ItoS || !z_q || !R || !dx || !chi2 || !applied) return UVIO_HP_E_ARG;
  if (mode != UVIO_HP_POSE_ORIENTATION && mode != UVIO_HP_POSE_FULL) return UVIO_HP_E_ARG;
  const bool full = mode == UVIO_HP_POSE_FULL;
  const int r = full ? 6 : 3;
  if ((full && !z_p) || ldr < r || N < 6 || ld < N || !(chi2_thr > 0.0)) return UVIO_HP_E_ARG;
  if (imu_id < 0 || (long long)imu_id + 6 > N) return UVIO_HP_E_ARG;
  auto clear = [&](int id, int lo, int len) { return (long long)id + 3 <= N && (id + 3 <= lo || id >= lo + len); };
  if (arm_id >= 0 && !clear(arm_id, imu_id, 6)) return UVIO_HP_E_ARG;
  if (rot_id >= 0 && (!clear(rot_id, imu_id, 6) || (arm_id >= 0 && !clear(rot_id, arm_id, 3)))) return UVIO_HP_E_ARG;
  if (!aux_upper_ok(R, ldr, r, true)) return UVIO_HP_E_ARG;
  DPoseState st{};
  bool finite = true;
  for (int k = 0; k < 4; k++) finite = finite && std::isfinite(st.q[k] = q[k]);
  for (int k = 0; k < 3; k++) finite = finite && std::isfinite(st.p[k] = p[k]) && std::isfinite(st.s[0][k] = s[k]);
  if (full)
    for (int k = 0; k < 3; k++) finite = finite && std::isfinite(st.zp[0][k] = z_p[k]);
  if (!finite || !unit_quat_ok(q_ItoS, st.qS[0]) || !unit_quat_ok(z_q, st.zq[0])) return UVIO_HP_E_ARG;
  for (int i = 0; i < r; i++)
    for (int j = i; j < r; j++) st.R[0][kChainMaxRows * i + j] = st.R[0][kChainMaxRows * j + i] = R[(size_t)i * ldr + j];
  st.thr[0] = chi2_thr;
  st.r[0] = r;
  st.id_arm[0] = (arm_id >= 0 && full) ? arm_id : -1;  // an orientation-only fix has no lever-arm columns
  st.id_rot[0] = rot_id >= 0 ? rot_id : -1;
  st.id_imu = imu_id;
  st.nf = 1;
  DevBuf<DPoseState> dst;
  DevBuf<DChainRow> drow;
  DevBuf<double> dM;
  DevBuf<unsigned char> dreg;
  std::vector<double> reg((size_t)N + kChainHeader, 0.0);
  const int rc = aux_standalone_run(P, (size_t)N, ld, [&](hipStream_t sm, double *dP) {
    dst = DevBuf<DPoseState>(1);
    drow = DevBuf<DChainRow>(1);
    dM = DevBuf<double>((size_t)kChainMaxRows * N);
    dreg = DevBuf<unsigned char>(sizeof(double) * reg.size());
    DChainRegion *region = chain_region(dreg, reg.size(), 0);
    HP_HIP(hipMemcpyAsync(dst, &st, sizeof(st), hipMemcpyHostToDevice, sm));
    HP_HIP(hipMemsetAsync(dreg, 0, sizeof(double) * reg.size(), sm));
    launch_pose_rows(sm, dst, 0, nullptr, drow, region);
    launch_chain_M(sm, dP, ld, N, drow, r, dM);
    launch_chain_update(sm, dP, ld, N, dM, drow, r, false, region);
    HP_HIP(hipMemcpyAsync(reg.data(), dreg, sizeof(double) * reg.size(), hipMemcpyDeviceToHost, sm));
  });
  if (rc) return rc;
  const DChainRegion g = chain_header(reg.data());
  *chi2 = g.chi2;
  *applied = g.accepted != 0.0 ? 1 : 0;
  for (int i = 0; i < N; i++) dx[i] = *applied ? reg[kChainHeader + i] : 0.0;
  if (g.extra != 0.0) return UVIO_HP_E_ARG;  // refused: S is not positive definite, nothing was applied
  if (*applied && g.neg > 0) return UVIO_HP_E_NUMERIC;
  return 0;
}

}  // namespace uvhp
