/*
 * uvio_hp.h — C ABI of the MI355X-native uvio/OpenVINS hot path
 * (track -> propagate -> MSCKF/SLAM/UWB update -> EKF update).
 *
 * This is the drop-in boundary.  The reference exposes C++ classes, not a C ABI
 * (SURVEY.md §8b); every entry point below names the reference interface it
 * replaces (path:line relative to the reference checkout).  All functions return
 * an int status: 0 = ok, < 0 = UVIO_HP_E_*.  They never call exit(); the
 * reference's fatal paths (std::exit on negative covariance diagonal,
 * StateHelper.cpp:112,181; propagation backwards, Propagator.cpp:39,46) become
 * UVIO_HP_E_NUMERIC / UVIO_HP_E_ORDER and leave the handle in a defined state.
 *
 * Threading (mirrors the reference, SURVEY §8b "Threading"): uvio_hp_feed_imu may be
 * called concurrently with the other feeds (IMU buffer is mutex-guarded like
 * Propagator::imu_data_mtx, Propagator.h:68), and so may uvio_hp_fast_state_propagate (it reads
 * a snapshot published by the feed thread); camera / sim / UWB feeds and every other call must be
 * serialized by the caller (single update thread, ROS1Visualizer.h:173).
 *
 * No torch / Eigen / OpenCV types cross this boundary: plain pointers and sizes.
 */
#ifndef UVIO_HP_H
#define UVIO_HP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UVIO_HP_OK 0
#define UVIO_HP_E_ARG (-1)      /* bad argument / size */
#define UVIO_HP_E_STATE (-2)    /* not initialized, or call not valid in this state; every state-changing call
                                   after a fatal error (E_NUMERIC / E_DEVICE / E_INTERNAL, where the reference
                                   std::exit's) returns it: the estimator is stopped, destroy the handle */
#define UVIO_HP_E_DEVICE (-3)   /* HIP runtime error or no MI355X device */
#define UVIO_HP_E_NUMERIC (-4)  /* negative covariance diagonal (ref: std::exit) */
#define UVIO_HP_E_CONFIG (-5)   /* config file missing / unparsable */
#define UVIO_HP_E_ORDER (-6)    /* measurement out of order (ref: std::exit in Propagator) */
#define UVIO_HP_E_CAPACITY (-7) /* a compile-time capacity was exceeded */
#define UVIO_HP_E_INTERNAL (-8) /* unexpected host-side error (a bug): the message names the routine */

#define UVIO_HP_MAX_CAMS 4
#define UVIO_HP_MAX_ANCHORS 16
#define UVIO_HP_AUX_MAX_DIM 8 /* scalars of one caller-defined state variable (uvio_hp_aux_add) */
/* uvio_hp_feed_pose's mode: the rows of a pose fix */
#define UVIO_HP_POSE_ORIENTATION 1 /* 3 rows: orientation only */
#define UVIO_HP_POSE_FULL 2        /* 6 rows: orientation, then position */
/* uvio_hp_debug_cov_propagate_p's path selector and the path it reports */
#define UVIO_HP_COV_PATH_AUTO 0  /* the engine's own rule */
#define UVIO_HP_COV_PATH_SPLIT 1 /* k_prop_T + k_prop_write (+ k_clone) */
#define UVIO_HP_COV_PATH_FUSED 2 /* k_prop_clone, or refuse */
/* uvio_hp_debug_cov_gather_p's kernel */
#define UVIO_HP_COV_MARGINALIZE 0       /* k_marginalize (m0, ms) */
#define UVIO_HP_COV_MARGINALIZE_MULTI 1 /* k_marginalize_multi (kept indices, ascending) */
#define UVIO_HP_COV_COMPACT 2           /* k_compact (kept indices) */
#define UVIO_HP_COV_MARGINAL_GATHER 3   /* k_marginal_gather (any indices) */

/* ---- option structs: the keys of estimator_config.yaml / kalibr_*.yaml / uwb_*.yaml ---- */

typedef struct {
  int model;       /* 0 = radtan (pinhole-radtan, CamRadtan.h), 1 = equidistant (CamEqui.h) */
  int width, height;
  double intrinsics[8]; /* fx fy cx cy d0 d1 d2 d3 (CamBase::set_value, CamBase.h:56) */
  double q_ItoC[4];     /* JPL quaternion of R_ItoC (x y z w), from T_imu_cam (VioManagerOptions.h) */
  double p_IinC[3];
} uvio_hp_camera_t;

typedef struct {
  uint64_t id;
  int fix;
  double p_AinG[3];
  double const_bias, dist_bias;
  double cov_diag[5]; /* p p p c d (UVioManagerOptions.h:80) */
} uvio_hp_anchor_t;

typedef struct {
  /* StateOptions (ov_msckf/src/state/StateOptions.h:41-96) */
  int do_fej;
  int integration;            /* 0 discrete, 1 rk4, 2 analytical */
  int num_cameras;
  int use_stereo;
  int do_calib_camera_pose;
  int do_calib_camera_intrinsics;
  int do_calib_camera_timeoffset;
  int do_calib_imu_intrinsics;
  int do_calib_imu_g_sensitivity;
  int imu_model;              /* 0 kalibr, 1 rpng */
  int max_clone_size;
  int max_slam_features;
  int max_slam_in_update;
  int max_msckf_in_update;
  int max_aruco_features;
  int feat_rep_msckf;         /* LandmarkRepresentation (LandmarkRepresentation.h:38), all six values 0-5; 5
                               * (ANCHORED_INVERSE_DEPTH_SINGLE) is linearized as 4, as UpdaterMSCKF does */
  int feat_rep_slam;          /* all six values 0-5; the state holds (x, y, z) for 0 and 2, (theta, phi, rho) for
                               * 1 and 3, (alpha, beta, rho) for 4 and rho alone for 5 (a one-dimensional landmark
                               * whose anchor bearing is kept in the handle); points: uvio_hp_get_features_slam */
  double dt_slam_delay;
  double gravity_mag;
  double calib_camimu_dt;
  /* UpdaterOptions (UpdaterOptions.h:33-44) */
  double msckf_sigma_pix, msckf_chi2_multipler;
  double slam_sigma_pix, slam_chi2_multipler;
  /* NoiseManager (Propagator.h:44) */
  double sigma_w, sigma_a, sigma_wb, sigma_ab;
  /* IMU intrinsics initial values (kalibr_imu_chain.yaml: Tw, Ta, Tg, R_IMUtoGYRO, R_IMUtoACC) */
  double imu_dw[6], imu_da[6], imu_tg[9];
  double q_GYROtoIMU[4], q_ACCtoIMU[4];
  /* FeatureInitializerOptions (FeatureInitializerOptions.h:33-70) */
  int fi_triangulate_1d, fi_refine_features, fi_max_runs;
  double fi_init_lamda, fi_max_lamda, fi_min_dx, fi_min_dcost, fi_lam_mult;
  double fi_min_dist, fi_max_dist, fi_max_baseline, fi_max_cond_number;
  /* cameras */
  uvio_hp_camera_t cams[UVIO_HP_MAX_CAMS];
  /* TrackKLT front-end (estimator_config.yaml: num_pts .. histogram_method) */
  int num_pts, fast_threshold, grid_x, grid_y, min_px_dist;
  int histogram_method;       /* 0 none, 1 histogram, 2 clahe */
  int downsample_cameras;     /* cams[].width/height/fx fy cx cy are the halved values (VioManagerOptions.h:251-260);
                               * camera feeds then take the raw 2 width x 2 height images */
  double track_frequency;
  /* uvio (UVioManagerOptions.h:52-90, UVioStateOptions.h:45, UVioUpdaterOptions.h:46) */
  int use_uwb;
  int do_calib_uwb_extrinsics;
  double prior_uwb_imu_cov;
  double uwb_sigma_range, uwb_chi2_multipler;
  double min_dist_to_use_uwb;
  double p_IinU[3];           /* uwb_extrinsics = -p_UinI */
  int n_anchors_to_fix;
  int n_anchors;
  uvio_hp_anchor_t anchors[UVIO_HP_MAX_ANCHORS];
  /* runtime */
  int record_timing;          /* per-frame stage timings (VioManager.cpp:631-644 schema); 1: host wall
                               * times + device event timing of the feature group, 2: also wait for the
                               * device at stage boundaries so each stage time includes its kernels */
  /* InertialInitializerOptions::init_max_features (InertialInitializerOptions.h:73): the KLT tracker
   * keeps floor(init_max_features / num_cameras) tracks per camera until an initializer succeeds
   * (VioManager.cpp:131; initialize_with_gt does not raise it to num_pts, VioManagerHelper.cpp:40) */
  int init_max_features;
  /* UpdaterZeroVelocity (VioManagerOptions.h:83-95, zupt_chi2_multipler :175) */
  int try_zupt;
  double zupt_chi2_multipler, zupt_max_velocity, zupt_noise_multiplier, zupt_max_disparity;
  int zupt_only_at_beginning;
  /* front-end selection (VioManagerOptions.h:440-452): the KLT front-end is the one implemented; use_klt = 0
   * (ORB descriptors) and use_aruco = 1 are rejected with UVIO_HP_E_CONFIG by uvio_hp_create */
  int use_klt, use_aruco;
  /* VioManagerOptions.h:98-101: per-frame timing rows in the reference CSV schema (VioManager.cpp:105-122,
   * 631-644); the file is recreated at uvio_hp_create */
  int record_timing_information;
  char record_timing_filepath[256];
  /* InertialInitializerOptions (InertialInitializerOptions.h:64-76): the static initializer's window (also
   * the IMU kept before initialization, VioManager.cpp:174-176), accelerometer excitation threshold, rest
   * disparity threshold; init_dyn_use selects the dynamic initializer, which is not built */
  double init_window_time, init_imu_thresh, init_max_disparity;
  int init_dyn_use;
  /* capacity reserved for caller-defined ("auxiliary") state variables (uvio_hp_aux_add): the sum of their
   * dimensions the covariance has room for.  0 (the default): none, and every buffer has the size it has without
   * the option.  Not a reference key; uvio_hp_options_load reads "max_aux_dim" if the file has it */
  int max_aux_dim;
} uvio_hp_options_t;

/* Per-frame stage timings in seconds, the reference CSV schema
 * "# timestamp (sec),tracking,propagation,msckf update,slam update,slam delayed,re-tri & marg,total"
 * (VioManager.cpp:117-121, rows :631-644). */
typedef struct {
  double timestamp;
  double tracking, propagation, msckf_update, slam_update, slam_delayed, marg, total;
  int n_msckf, n_slam, n_slam_delayed, n_clones, cov_dim;
  int msckf_rows;   /* stacked rows m before compression */
  int msckf_cols;   /* H columns n */
  /* not filled (always zero): kept so the struct layout does not change.  The per-feature linearize kernel's
   * launches, seconds and FLOPs are in the "feature" class of uvio_hp_get_kernel_stats */
  int k_feat_launches;
  double k_feat_s;
  double k_feat_flops;
  /* host waits on the device during this frame (tracker + estimator): count and seconds blocked */
  int device_syncs;
  double sync_wait;
  int zupt;  /* 1: this frame ended in a zero-velocity update (UpdaterZeroVelocity::try_update accepted) */
  int n_anchor_change;  /* SLAM landmarks re-anchored by UpdaterSLAM::change_anchors this frame (UpdaterSLAM.cpp:481-503) */
  /* the per-frame device update chain (MSCKF, SLAM chunks, delayed initialization enqueued back to back, DESIGN.md
   * §4): seconds of its single wait for the device plus the host replay of the results.  The chain books this
   * time in slam_delayed (the last stage); msckf_update / slam_update hold the host enqueue times of theirs */
  double chain_wait;
  /* upload staging ring this frame: restarts of the ring (each waits for the device), and 1 when
   * the update chain's state blob had to be copied out of the ring's previous epoch (engine_chain.cpp) */
  int stage_restarts;
  int chain_blob_old_epoch;
} uvio_hp_timing_t;

/* Live device timing of the kernel classes the benchmark prices against a roofline (HIP events on the
 * library stream around each launch of the class): cumulative since the timing was
 * switched on.  bound: 0 = HBM bandwidth (bytes), 1 = FP64 matrix / vector peak (flops); flops / bytes are
 * the ALGORITHMIC counts of the launches; kernels = the kernel names of the class as
 * rocprofv3 reports them (comma separated). */
typedef struct {
  char name[24];
  char kernels[192];
  int bound;
  long long launches;
  double seconds, flops, bytes;
} uvio_hp_kstat_t;

typedef struct uvio_hp uvio_hp_t;

/* ---- options ---- */
/* Defaults of the reference option structs (StateOptions.h, UpdaterOptions.h, ...). */
int uvio_hp_options_default(uvio_hp_options_t *opts);
/* Parse estimator_config.yaml (+ relative_config_imu / relative_config_imucam / config_uwb files)
 * with the reference's keys (YamlParser, opencv_yaml_parse.h:65-163; VioManagerOptions::print_and_load).
 * Only the keys present in the files are written: call uvio_hp_options_default on the struct first (as
 * the reference's option structs start from their defaults). */
int uvio_hp_options_load(const char *estimator_config_path, uvio_hp_options_t *opts);

/* ---- lifetime ---- */
/* replaces ov_msckf::VioManager::VioManager(VioManagerOptions&) (VioManager.cpp:50) and
 * uvio::UVioManager::UVioManager (uvio/src/core/UVioManager.cpp:26). device = HIP ordinal. */
int uvio_hp_create(const uvio_hp_options_t *opts, int device, uvio_hp_t **out);
int uvio_hp_destroy(uvio_hp_t *h);
/* message of the last failed call on h; with h == NULL, why the last uvio_hp_create on this thread failed */
const char *uvio_hp_last_error(const uvio_hp_t *h);

/* ---- feeds (VioManager.h:75-96, UVioManager.h:48-60) ---- */
/* VioManager::initialize_with_gt(Matrix<17,1>) (VioManagerHelper.cpp:40): x = [t, q_GtoI(4), p, v, bg, ba] */
int uvio_hp_initialize_with_gt(uvio_hp_t *h, const double x[17]);
/* VioManager::feed_measurement_imu (VioManager.cpp:166) */
int uvio_hp_feed_imu(uvio_hp_t *h, double t, const double wm[3], const double am[3]);
/* n consecutive feed_measurement_imu calls in one: t[n], wm[3n], am[3n] (a driver that receives IMU
 * samples in bursts between camera frames saves the per-call overhead) */
int uvio_hp_feed_imu_batch(uvio_hp_t *h, int n, const double *t, const double *wm, const double *am);
/* VioManager::feed_measurement_simulation (VioManager.cpp:191) — TrackSIM path.  For camera i
 * (i < ncam) there are counts[i] features; ids/uv are concatenated over cameras, uv as (u,v) pairs. */
int uvio_hp_feed_simulation(uvio_hp_t *h, double t, int ncam, const int *cam_ids, const int *counts,
                            const uint64_t *ids, const float *uv);
/* VioManager::feed_measurement_camera / UVioManager::feed_measurement_camera (UVioManager.h:48).
 * imgs[i] is a u8 W x H image with row stride strides[i]; masks may be NULL.
 * W x H is the camera's configured size (with downsample_cameras the image is 2W x 2H).  No shape is refused:
 * the sides need no divisibility, the cameras of one feed (a stereo pair included) may differ in size and
 * so in pyramid depth, and strides[i] >= the image's width is the only requirement on the rows (E_ARG
 * otherwise), with any alignment.  Tested from 31 x 31 and 90 x 30 up ("Image shapes");
 * CLAHE needs sides >= 9, and a grid cell (W / grid_x by H / grid_y) below 7 x 7 pixels yields no corner. */
int uvio_hp_feed_camera(uvio_hp_t *h, double t, int ncam, const int *cam_ids, const uint8_t *const *imgs,
                        const int *strides, const uint8_t *const *masks);
/* The same with imgs[i] in device memory (HBM-resident input, e.g. a camera DMA buffer or a torch
 * tensor); the images must be complete (their producer synchronized) before the call.  masks stay
 * host pointers. */
int uvio_hp_feed_camera_device(uvio_hp_t *h, double t, int ncam, const int *cam_ids, const uint8_t *const *imgs,
                               const int *strides, const uint8_t *const *masks);
/* UVioManager::feed_measurement_uwb (UVioManager.cpp:61): one UwbData message */
int uvio_hp_feed_uwb(uvio_hp_t *h, double t, int n, const uint64_t *anchor_ids, const double *ranges);
/* UVioManager::try_to_initialize_uwb_anchors (UVioManager.cpp:81) */
int uvio_hp_init_anchors(uvio_hp_t *h, int n, const uvio_hp_anchor_t *anchors);

/* ---- getters (VioManager.h:99-111) ---- */
int uvio_hp_initialized(const uvio_hp_t *h, int *out);
/* IMU value [q(4) p(3) v(3) bg(3) ba(3)] and the state time */
int uvio_hp_get_imu_state(uvio_hp_t *h, double *t, double out[16]);
/* covariance dimension N (State::max_covariance_size, State.h:88) */
int uvio_hp_get_cov_dim(uvio_hp_t *h, int *n);
/* dense N x N covariance into out with leading dimension ld (row-major) */
int uvio_hp_get_cov(uvio_hp_t *h, double *out, int ld);
/* the state mean in State::_variables order (each variable's value(): quat 4 + ...);
 * *len receives the number of doubles written; meta (optional, 3 ints per variable:
 * kind, covariance id, covariance size) */
int uvio_hp_get_state_vector(uvio_hp_t *h, double *out, int cap, int *len, int *meta, int meta_cap, int *nvars);
/* the first-estimate (FEJ) values, same layout as uvio_hp_get_state_vector (Type::fej(), Type.h:87) */
int uvio_hp_get_fej_vector(uvio_hp_t *h, double *out, int cap, int *len);
/* timings of the last processed frame */
int uvio_hp_get_timing(uvio_hp_t *h, uvio_hp_timing_t *out);
/* live per-class kernel timing: 0 = off (default), k > 0 = the launches of every k-th camera / simulated
 * frame are timed (each timed launch costs two event records on the host) */
int uvio_hp_set_kernel_timing(uvio_hp_t *h, int period);
/* the per-class statistics (*n receives the number of classes); flush = 1 waits for the device first so
 * every launch enqueued so far is counted */
int uvio_hp_get_kernel_stats(uvio_hp_t *h, int flush, uvio_hp_kstat_t *out, int cap, int *n);
/* VioManager::get_active_tracks (VioManager.h:114, filled by retriangulate_active_tracks,
 * VioManagerHelper.cpp:190-388): the current tracks' positions p_FinG (3 per track) and, for the tracks seen
 * by camera 0 in front of it and inside its image, (u, v, depth) (3 per track, uvd_valid 1); *t receives
 * active_tracks_time.  *n receives the number of tracks (E_CAPACITY if > cap). */
int uvio_hp_get_active_tracks(uvio_hp_t *h, double *t, uint64_t *ids, double *posinG, double *uvd, int *uvd_valid,
                              int cap, int *n);
/* VioManager::get_features_SLAM (VioManagerHelper.cpp:417-438): every SLAM landmark of the state as a point in the
 * global frame (3 per landmark), in the order of the landmarks' variables in the state vector; an anchored
 * representation is transformed through its anchor clone and anchor camera.  With an inverse-depth feat_rep_slam
 * the state vector holds (theta, phi, rho), (alpha, beta, rho) or a lone rho per landmark, not a point: read
 * points here.
 * *n receives the number of landmarks (E_CAPACITY if > cap). */
int uvio_hp_get_features_slam(uvio_hp_t *h, uint64_t *ids, double *xyz_inG, int cap, int *n);
/* number of clones and their timestamps (ascending) */
int uvio_hp_get_clone_times(uvio_hp_t *h, double *out, int cap, int *n);
/* TrackBase::get_last_obs / get_last_ids (TrackBase.h:137-148) for one camera: ids and raw (u, v) of
 * the KLT tracks after the last camera feed; *n receives the count (E_CAPACITY if > cap) */
int uvio_hp_get_tracks(uvio_hp_t *h, int cam, uint64_t *ids, float *uv, int cap, int *n);
/* the last image pyramid of one camera (TrackKLT::img_pyramid_last, TrackKLT.h:147): level size,
 * the (equalized) u8 image (w*h) and interleaved Scharr (dx, dy) int16 derivatives (w*h*2); img / der
 * may be NULL, cap = pixels available */
int uvio_hp_get_pyramid(uvio_hp_t *h, int cam, int level, int *w, int *hgt, uint8_t *img, int16_t *der, size_t cap);
/* StateHelper::get_marginal_covariance (StateHelper.cpp:226-254): block k is the variable with covariance id
 * ids[k] and size sizes[k] (uvio_hp_get_state_vector's meta); out is m x m, m = sum sizes, leading dimension ld.
 * The blocks may come in any order and may repeat (the reference copies whatever list it is given).  The rows
 * and columns are gathered on the device into a dense block and only that block is copied back (the pose
 * covariance of ROS1Visualizer.cpp:618, 805 is 36 numbers of an N x N matrix).  nvar == 0 does nothing.
 * UVIO_HP_E_ARG: null pointers, nvar < 0, a size < 1, a block outside [0, N), ld < m; UVIO_HP_E_CAPACITY: m above
 * the covariance capacity; every check comes before any device work, and a refused call leaves out untouched.
 * Serialized with the feeds, like the other getters. */
int uvio_hp_get_marginal_cov(uvio_hp_t *h, int nvar, const int *ids, const int *sizes, double *out, int ld);
/* VioManager::get_good_features_MSCKF (VioManager.h:123, filled at VioManager.cpp:555-570): p_FinG (3 per feature)
 * of the features the frame's MSCKF update kept, in the update's order (the status-0 entries of
 * uvio_hp_debug_last_msckf).  As in the reference the list is cleared only by a frame whose first camera id is 0
 * and appended to otherwise.  *n receives the number of features (E_CAPACITY if > cap). */
int uvio_hp_get_good_features_msckf(uvio_hp_t *h, double *xyz_inG, int cap, int *n);
/* switch the odometry cache on / off (off by default).  On: the calls after which the reference invalidates its
 * cache (Propagator::invalidate_cache: VioManager.cpp:230, 303, 526, 543, UVioManager.cpp:161 -- a frame that ends
 * in a zero-velocity update or reaches its update stage, uvio_hp_msckf_update, uvio_hp_slam_update) and the calls
 * that set the state (uvio_hp_initialize_with_gt, a static initialization, uvio_hp_set_state, this call; an applied
 * uvio_hp_measurement_update, which has no counterpart inside the reference and is treated as an update) publish
 * the IMU state, its 15 x 15 marginal, calib_camimu_dt and the IMU intrinsics as the cache's next content: one
 * 15 x 15 device gather and a 1.8 KB copy per such call, no host wait.  A frame that returns before its update
 * stage, a propagation, a delayed initialization, uvio_hp_uwb_update_single and the marginalization calls leave the
 * cache alone, as the reference does.  Serialized with the feeds. */
int uvio_hp_odometry_enable(uvio_hp_t *h, int on);
/* Propagator::fast_state_propagate (Propagator.cpp:140-267; ROS1Visualizer::visualize_odometry,
 * ROS1Visualizer.cpp:245-327): state_plus = [q_GtoI(4) p_IinG(3) v_IinI(3) w_IinI(3)],
 * cov 12 x 12 row-major in the reference's order (theta, p, v local, w); *ok = 0 where the reference returns false
 * (fewer than two IMU readings for the interval: state_plus and cov are left untouched).  The cache is left at t
 * with a zero time offset, so successive queries chain, as in the reference.
 * Threading: may be called from any thread beside every other call on the handle (the IMU callback's thread,
 * ROS1Visualizer.cpp:67).  A query that arrives while a frame is running uses the previous cache; the first query
 * after the frame adopts the snapshot the frame published (the reference reads the live state inside that query
 * instead, racing with the update thread).  The IMU intrinsics (Dw, Da, Tg, R_ACCtoIMU, R_GYROtoIMU) are taken with
 * the snapshot, where the reference reads them live on every call: the two differ only after a state change that
 * did not invalidate the cache.
 * UVIO_HP_E_STATE: the cache is off, or the filter is not initialized.  The call does not set uvio_hp_last_error. */
int uvio_hp_fast_state_propagate(uvio_hp_t *h, double t, double state_plus[13], double cov[144], int *ok);

/* ---- image products ("Image products") ---- */
/* VioManager::get_historical_viz_image (VioManagerHelper.cpp:389-415): the canvas of TrackBase::display_history
 * (TrackBase.cpp:119-228) called with the colours (255, 255, 0) / (255, 255, 255) and the SLAM landmarks of the state
 * as the highlighted ids, rendered on the device over level 0 of the last pyramids.  The canvas is 3-channel 8-bit,
 * packed, row-major, *height x *width pixels: max_h x (ncam * max_w) over the cameras of the last camera feed in
 * ascending camera id, camera k at x offset k * max_w.  Before the first camera feed *width = *height = 0 (the
 * reference returns an empty cv::Mat) and nothing is written.  out == NULL only reports the size; otherwise cap is
 * the bytes available (UVIO_HP_E_CAPACITY if fewer than 3 * *width * *height, with the size reported).
 * *overlay names the text the reference would put on each camera's image: 0 = "CAM:k", 1 = "init" (not
 * initialized), 2 = "zvupt" (the last frame ended in a zero-velocity update).  The glyphs themselves are NOT drawn:
 * cv::putText needs OpenCV's Hershey font tables, which this library does not carry; an adapter that has OpenCV adds
 * the text with one cv::putText per camera (position, scale and colour: TrackBase.cpp:213-219).  The image is always
 * built from scratch (the reference's "draw on top of the previous image" branch is not reproduced); the drawing
 * rules are listed in DESIGN.md.  Nothing is kept, copied or enqueued per frame for this call: it costs the feeds
 * nothing unless it is made.  Serialized with the feeds, like the other getters. */
int uvio_hp_get_track_image(uvio_hp_t *h, uint8_t *out, size_t cap, int *width, int *height, int *overlay);
/* the same with out in device memory (a torch tensor, a GPU encoder's input): the call returns with the image
 * complete */
int uvio_hp_get_track_image_device(uvio_hp_t *h, uint8_t *out, size_t cap, int *width, int *height, int *overlay);
/* Feature::uvs[cam] of feature id as the handle's database holds it, oldest first ((u, v) pairs, the first cap
 * of them written; UVIO_HP_E_CAPACITY if *n > cap), how many cameras have seen the feature (Feature::uvs.size(),
 * display_history's is_stereo test) and Feature::to_delete.  *n = 0 (and *n_cams = 0) when the feature is unknown.
 * n_cams / to_delete may be NULL.  This is what an adapter needs to draw the tracks in a style of its own. */
int uvio_hp_get_track_history(uvio_hp_t *h, int cam, uint64_t id, float *uv, int cap, int *n, int *n_cams,
                              int *to_delete);
/* The two images of ROS1Visualizer::publish_loopclosure_information (ROS1Visualizer.cpp:950-996) for camera 0, both
 * *height x *width (camera 0's size): depth, the 16-bit map, zero except at ((int)v, (int)u) of every active track
 * (uvio_hp_get_active_tracks, uvd_valid 1) whose (u, v) passes the function's border test (dw = 4), where it holds
 * (uint16_t)(1000 * depth) (the low 16 bits of the truncated integer); viz (3 channels, packed), camera 0's last
 * image (pyramid level 0) with the filled square of half-side dw per such track in the function's inverse-depth
 * colour ramp.  The tracks are drawn in ascending feature id (the reference iterates an unordered_map: its order,
 * and so which of two overlapping squares wins, is unspecified there).  Either pointer may be NULL; cap = pixels
 * available in each given buffer (depth: cap uint16_t, viz: 3 * cap bytes; UVIO_HP_E_CAPACITY otherwise, with the
 * size reported).  *t receives active_tracks_time (-1, with a zero size, before the first retriangulation or camera
 * feed). */
int uvio_hp_get_loop_depth(uvio_hp_t *h, uint16_t *depth, uint8_t *viz, size_t cap, int *width, int *height, double *t);

/* ---- Updater-level boundary: one updater call on the handle's current state ----
 * These mirror the reference's Updater C++ surfaces for a caller that keeps its own feature database
 * (the feeds above run the whole VioManager frame instead).  Features come as flat arrays: feature i has
 * id featids[i] and the measurements meas[meas_off[i] .. meas_off[i+1]) in the order they were observed
 * (the order FeatureDatabase::update_feature appended them, FeatureDatabase.cpp:59-98); a camera's track
 * is created at its first measurement, which reproduces ov_core::Feature's per-camera map order.  The
 * results (one record per input feature) say what the reference leaves on the Feature and in
 * feature_vec.  The covariance never leaves the device; each call reads back only dx. */
typedef struct {
  int cam;          /* camera id */
  double t;         /* Feature::timestamps[cam] entry */
  float u, v;       /* Feature::uvs[cam] entry (raw pixel) */
  float un, vn;     /* Feature::uvs_norm[cam] entry (undistorted, normalized) */
} uvio_hp_feat_meas_t;

typedef struct {
  uint64_t featid;
  int status;       /* 0 used by the update (kept in feature_vec); 1 too few measurements or triangulation failed;
                     * 2 Gauss-Newton refinement failed; 3 chi2 rejected (all but 0 are erased from feature_vec) */
  int to_delete;    /* Feature::to_delete after the call */
  double p_FinG[3]; /* the triangulated position (MSCKF / delayed init; zero when not triangulated) */
  double chi2;      /* the chi2 the gate compared (0 when not gated) */
} uvio_hp_feat_result_t;

/* Overwrite the mean, the first estimates and the covariance (a state snapshot in the layout of
 * uvio_hp_get_state_vector / uvio_hp_get_fej_vector / uvio_hp_get_cov: same variables, len doubles,
 * N x N covariance with leading dimension ld).  Camera intrinsics follow the state (StateHelper.cpp:190-195).
 * The anchor bearings of ANCHORED_INVERSE_DEPTH_SINGLE landmarks are not part of the vector: the handle keeps
 * the ones it has, so a snapshot is only meaningful for the handle (or a copy of the run) it was taken from. */
int uvio_hp_set_state(uvio_hp_t *h, const double *val, const double *fej, int len, const double *P, int N, int ld);
/* Propagator::propagate_and_clone (Propagator.h:110) to t with the IMU readings fed so far */
int uvio_hp_propagate_and_clone(uvio_hp_t *h, double t);
/* UpdaterMSCKF::update (UpdaterMSCKF.h:68, UpdaterMSCKF.cpp:58-295).
 * UVIO_HP_E_CAPACITY, before the batch's kernels (covariance and state untouched, the handle stays usable): a feature of
 * more than 64 measurements; a batch whose largest measurement count and widest per-feature Jacobian, taken
 * together, need more LDS than the feature kernel has (e.g. 60 measurements of a feature over 30 clones of a
 * calibrated stereo pair, or a 64-measurement feature in one batch with a feature over 25 clones); 512 or more
 * state columns in one batch.  uvio_hp_slam_update's batches pass the same check. */
int uvio_hp_msckf_update(uvio_hp_t *h, int nfeat, const uint64_t *featids, const int *meas_off,
                         const uvio_hp_feat_meas_t *meas, uvio_hp_feat_result_t *out);
/* UpdaterSLAM::update (UpdaterSLAM.h:70, UpdaterSLAM.cpp:253-479); every feature must be a SLAM landmark of
 * the state (UVIO_HP_E_ARG otherwise); a chi2 rejection raises the landmark's fail count as in the reference */
int uvio_hp_slam_update(uvio_hp_t *h, int nfeat, const uint64_t *featids, const int *meas_off,
                        const uvio_hp_feat_meas_t *meas, uvio_hp_feat_result_t *out);
/* UpdaterSLAM::delayed_init (UpdaterSLAM.h:77, UpdaterSLAM.cpp:61-251): accepted features (status 0) become
 * SLAM landmarks of the state in the configured feat_rep_slam */
int uvio_hp_slam_delayed_init(uvio_hp_t *h, int nfeat, const uint64_t *featids, const int *meas_off,
                              const uvio_hp_feat_meas_t *meas, uvio_hp_feat_result_t *out);
/* UpdaterSLAM::change_anchors (UpdaterSLAM.h:87, UpdaterSLAM.cpp:481-647) */
int uvio_hp_slam_change_anchors(uvio_hp_t *h);
/* StateHelper::marginalize_slam / marginalize_old_clone (StateHelper.h:230, :224) */
int uvio_hp_marginalize_slam(uvio_hp_t *h);
int uvio_hp_marginalize_old_clone(uvio_hp_t *h);
/* UpdaterUWB::update_single (UpdaterUWB.h:55, UpdaterUWB.cpp:53-90): one range to one initialized anchor on
 * the current state (t is the measurement time; the reference's Jacobian does not use it); *applied = 1
 * when the chi2 test passed and the update ran, 0 when it was gated or the anchor is unknown */
int uvio_hp_uwb_update_single(uvio_hp_t *h, double t, uint64_t anchor_id, double range, int *applied);

/* ---- a measurement of the caller's own (GPS / mocap position, barometer, wheel odometry, magnetometer ...) ----
 * The two reference surfaces uvio itself used to add UWB from outside the estimator: move the filter to the
 * measurement's time, then one StateHelper::EKFUpdate with the caller's Jacobian, residual and noise matrix.
 * The sequence is propagate -> uvio_hp_get_state_vector (values and meta) -> build H and res -> update. */
/* UVioPropagator::propagate (UVioPropagator.cpp:27-115): the state and covariance to time t (IMU clock) with the
 * IMU readings fed so far, without a clone.  The reference's two quirks are kept: the end time carries no
 * camera-IMU time offset, and last_prop_time_offset is not updated.  UVIO_HP_E_ORDER when t is not after the
 * state time (the state is untouched), UVIO_HP_E_STATE before initialization.  The odometry cache is left alone,
 * as by uvio_hp_propagate_and_clone. */
int uvio_hp_propagate(uvio_hp_t *h, double t);
/* StateHelper::EKFUpdate(state, H_order, H, res, R) (StateHelper.h:88, StateHelper.cpp:116-197) behind the chi2
 * test of UpdaterUWB.cpp:67-79.  H_order is the block list: block k of H's columns is the covariance range
 * [ids[k], ids[k] + sizes[k]) (uvio_hp_get_state_vector's meta; any order, repeats allowed, as for
 * uvio_hp_get_marginal_cov).  H is r x n (row-major, leading dimension ldh), n = sum sizes, with respect to the
 * error state: the JPL left quaternion error for orientations, each landmark's own parametrization.  res is the
 * r residuals, R the r x r noise matrix (leading dimension ldr) of which only the upper triangle is read
 * (S.triangularView<Upper>() += R, StateHelper.cpp:156).
 * Gate: S = H P_II H^T + R, chi2 = res^T S^-1 res; the update runs iff chi2 is not above chi2_thr (INFINITY: no
 * gate; for the reference's updaters chi2_thr = chi2_multipler * uvio_hp_chi2_95(r)).  Accepted: the covariance is
 * updated on the device (P -= (M L^-T)(M L^-T)^T, S = L L^T, the kernels of every other update) and dx = K res
 * moves the mean through Type::update (values only; first estimates stay).  One readback, one host wait.
 * *chi2 and *applied are written whenever the call returns 0; dx (optional, N doubles, N = uvio_hp_get_cov_dim)
 * receives the correction, zeros when the update was not applied.  r == 0 or nvar == 0 does nothing (*applied = 0).
 * UVIO_HP_E_ARG, before any device work: null pointers, nvar < 0, a size < 1, a block outside [0, N), ldh < n,
 * ldr < r, a chi2_thr that is not positive (or NaN), a non-finite entry of H, res or the read triangle of R.
 * UVIO_HP_E_CAPACITY, before any device work: r > 255 rows or n > 1215 columns (uvio_hp_ekf_update's limits), or
 * an H larger than the upload staging ring.
 * UVIO_HP_E_ARG after the factorization: S is not positive definite (a pivot of its LDL^T factor is not a finite
 * positive number; uvio_hp_last_error says so); covariance and mean are untouched and the handle stays usable.
 * UVIO_HP_E_NUMERIC (fatal, as everywhere): a negative covariance diagonal after an accepted update.
 * Serialized with the feeds.  When applied the odometry cache is republished, as after uvio_hp_msckf_update.
 * A state variable of the caller's own (a sensor bias, a lever arm) is added with uvio_hp_aux_add below and named
 * here like any other block.  A position fix or a pose fix can instead be buffered inside the frame and relinearized on
 * the device (uvio_hp_feed_position, uvio_hp_feed_pose below); for any other model this call, after
 * uvio_hp_propagate, is the one to use. */
int uvio_hp_measurement_update(uvio_hp_t *h, int nvar, const int *ids, const int *sizes, const double *H, int ldh, int r,
                               const double *res, const double *R, int ldr, double chi2_thr, double *chi2, int *applied,
                               double *dx);

/* ---- state variables of the caller's own ("auxiliary" states: a lever arm, a sensor bias, a frame offset, a scale) ----
 * Small additive vectors (1 .. UVIO_HP_AUX_MAX_DIM scalars, updated as value += dx like ov_type::Vec) appended to
 * the running estimator the way uvio appends p_IinU and its anchors (StateHelper::set_initial_covariance,
 * StateHelper.cpp:199-223; StateHelper::initialize_invertible, StateHelper.cpp:484-577), but on the device: the new
 * rows and columns of the covariance are written in place, nothing is copied to the host.  The options' max_aux_dim
 * reserves the room.  A variable shows in uvio_hp_get_state_vector's meta as kind 6 and is named in
 * uvio_hp_measurement_update / uvio_hp_get_marginal_cov by its covariance offset, which MOVES when clones or
 * landmarks in front of it are marginalized: ask uvio_hp_aux_get for the offset before building an H.  The handle
 * (a positive int) stays valid until uvio_hp_aux_remove.  With feature sharding every rank must add the same
 * variables at the same points of the stream.
 * Refusals come before any device work and leave the state and the covariance untouched: UVIO_HP_E_STATE before
 * initialization; UVIO_HP_E_ARG for a null pointer, dim outside 1 .. 8, a block outside [0, N), a leading dimension
 * below the row length, a non-finite input, a prior diagonal that is not positive, a negative walk_sigma, a singular
 * H_aux, a dead handle; UVIO_HP_E_CAPACITY when the live aux dimensions plus dim exceed max_aux_dim, or H_x has more
 * than 1215 columns.  Serialized with the feeds. */
/* A variable with value val[dim] and the prior covariance prior_cov (dim x dim, leading dimension ld; only the upper
 * triangle is read, as for R), uncorrelated with everything else.  walk_sigma[dim] (NULL: all zero, a constant) is
 * the continuous-time random-walk density of each component in unit / sqrt(s): wherever the state time advances by
 * dt (a camera frame's propagation, uvio_hp_propagate, a UWB message, a zero-velocity update) the component's
 * variance grows by walk_sigma^2 * dt. */
int uvio_hp_aux_add(uvio_hp_t *h, int dim, const double *val, const double *prior_cov, int ld, const double *walk_sigma,
                    int *handle);
/* StateHelper::initialize_invertible for a caller's variable: dim rows of a measurement
 * res = H_x dx + H_aux dx_aux + noise(R) with H_x (dim x n, leading dimension ldhx) over the blocks
 * [ids[k], ids[k] + sizes[k]) as in uvio_hp_measurement_update (nvar may be 0), an invertible H_aux (dim x dim,
 * ldha) and a dense R (dim x dim, ldr, upper triangle read).  The value becomes val0 + H_aux^-1 res, the
 * cross-covariance -P[:, I] H_x^T H_aux^-T and the variable's own block H_aux^-1 (H_x P_II H_x^T + R) H_aux^-T.
 * H_aux^-1 is formed on the host (Gauss-Jordan, partial pivoting; a pivot not above dim * 2^-52 * max |H_aux| is
 * singular). */
int uvio_hp_aux_add_from_measurement(uvio_hp_t *h, int dim, const double *val0, int nvar, const int *ids,
                                     const int *sizes, const double *H_x, int ldhx, const double *H_aux, int ldha,
                                     const double *res, const double *R, int ldr, const double *walk_sigma,
                                     int *handle);
/* A JPL unit quaternion [x y z w] of the caller's own (a sensor's mounting rotation): 4 values, 3 error dimensions,
 * updated as q <- dq(dtheta) (x) q with dq = normalize([dtheta / 2, 1]) (ov_type::JPLQuat::update), by every path that
 * corrects the state: uvio_hp_measurement_update on its 3 columns, the frame's updates, UWB, zero-velocity, position
 * and pose fixes.  Value and first estimate are set together.  q is normalized on entry; UVIO_HP_E_ARG when it is not
 * finite or its norm lies outside [0.5, 2].  prior_cov is 3 x 3 (leading dimension ld >= 3, upper triangle read) over
 * the error dtheta, walk_sigma[3] (NULL: a constant) in rad / sqrt(s).  The variable shows in
 * uvio_hp_get_state_vector's meta as kind 7, size 3, and contributes 4 doubles to the value and first-estimate
 * vectors; it counts 3 against max_aux_dim.  Every other refusal, their order (before any device work) and the
 * sharding note are uvio_hp_aux_add's. */
int uvio_hp_aux_add_quat(uvio_hp_t *h, const double q[4], const double *prior_cov, int ld, const double walk_sigma[3],
                         int *handle);
/* the variable's current covariance offset, its dimension and its value (val: dim doubles, may be NULL).  For a
 * quaternion variable (uvio_hp_aux_add_quat) *dim = 3 and val receives 4 doubles: give val room for
 * UVIO_HP_AUX_MAX_DIM doubles whenever the kind is not known. */
int uvio_hp_aux_get(uvio_hp_t *h, int handle, int *id, int *dim, double *val);
/* StateHelper::marginalize of the variable; the handle is dead afterwards */
int uvio_hp_aux_remove(uvio_hp_t *h, int handle);
/* number of live aux variables and the sum of their dimensions (either pointer may be NULL) */
int uvio_hp_aux_count(uvio_hp_t *h, int *n, int *dims_used);

/* ---- buffered position fixes (GPS / mocap position, an altimeter, a planar positioning system) ----
 * What the reference does for its UWB messages (UVioManager.cpp:178-188), for the commonest external measurement:
 * a fix is queued, and the next uvio_hp_feed_camera / _simulation propagates to each queued time in (state time,
 * frame time) and updates there, merged in ascending time with the buffered UWB messages (at equal times the UWB
 * message first, then the fixes in feed order).  The model is a position fix of a sensor point S on the body,
 *     z = C (p_IinG + R_GtoI^T s) + noise(R),
 * r = 1 .. 3 rows, C r x 3 row-major (I: GPS / mocap; e_z^T: an altimeter; two rows: planar), R r x r (leading
 * dimension ldr, upper triangle read), s the constant lever arm p_SinI[3] (aux_handle <= 0) or a live 3-dimensional
 * aux variable (aux_handle > 0; p_SinI is then ignored and may be NULL) whose value and covariance offset are
 * looked up at replay.  H over the error state is C [-R_GtoI^T [s]x | I | R_GtoI^T] (JPL left error), the last
 * block only for an aux lever arm.  Each distinct time runs uvio_hp_propagate's propagation (both quirks, the aux
 * random walk); the fixes of one time then form one device chain with one readback per 8 fixes, each fix linearized at
 * the state the previous one left.  Gate: chi2_mult * uvio_hp_chi2_95(r) (chi2_mult = INFINITY: no gate).
 * t is in the clock uvio_hp_propagate takes.  *queued = 0 with a return of 0 when the filter is not initialized or t is
 * not after the state time (uvio_hp_feed_uwb's behaviour).  UVIO_HP_E_ARG, before anything is stored: null pointers,
 * r outside 1 .. 3, ldr < r, a non-finite t, C, z, read triangle of R or p_SinI, a diagonal of R that is not positive,
 * a chi2_mult that is not positive (or NaN), an aux handle that is dead or not 3-dimensional.  UVIO_HP_E_CAPACITY: 256
 * fixes are already queued (host memory).  A frame that ends in a zero-velocity update leaves the queue alone; fixes
 * at or before the frame time are erased afterwards.  UVIO_HP_E_NUMERIC (fatal) from the frame: a negative covariance
 * diagonal after an applied fix.  Serialized with the feeds; with feature sharding every rank makes the call. */
int uvio_hp_feed_position(uvio_hp_t *h, double t, int r, const double *C, const double *z, const double *R, int ldr,
                          const double *p_SinI, int aux_handle, double chi2_mult, int *queued);
/* The fixes consumed by the last camera or simulation feed, in processing order: time, chi2 and status (any array may
 * be NULL).  Status 0: applied.  1: gated (chi2 above the threshold).  2: dropped (its time was not after the state time
 * at replay, or equal to the frame time, or the propagation to it failed for lack of IMU readings).  3: refused (S not
 * positive definite or a NaN chi2, or the aux handle was removed after queueing); the state is untouched.
 * *n is always written; UVIO_HP_E_CAPACITY when *n > cap (nothing else is written). */
int uvio_hp_get_position_results(uvio_hp_t *h, double *t, double *chi2, int *status, int cap, int *n);

/* ---- buffered pose fixes (motion capture, a dual-antenna GNSS/INS, a fiducial localizer) ----
 * The rotation twin of uvio_hp_feed_position.  A sensor frame S is rigidly mounted on the body with the rotation q_ItoS
 * and the lever arm s = p_SinI; an external system reports S's pose in the filter's global frame G: z_q = q_GtoS (JPL,
 * [x y z w]) and z_p = p_SinG.  The caller aligns the frames, as for uvio_hp_feed_position (a filter started with
 * uvio_hp_initialize_with_gt from the same system already has G equal to its frame).  With the JPL left error for both
 * quaternions, R_GtoI = (I - [dtheta]x) R^_GtoI and R_ItoS = (I - [dphi]x) R^_ItoS, the prediction is
 * q^_GtoS = q^_ItoS (x) q^_GtoI and p^ = p_IinG + R_GtoI^T s, and
 *     orientation rows: dq = z_q (x) inv(q^_GtoS), negated when dq.w < 0; r_theta = 2 dq.xyz;
 *                       H over [dtheta, dp, ds, dphi] = [ R^_ItoS | 0 | 0 | I ]
 *     position rows:    r_p = z_p - p^;  H = [ -R_GtoI^T [s]x | I | R_GtoI^T | 0 ]
 * mode UVIO_HP_POSE_ORIENTATION: r = 3 rows (z_p, p_SinI and the lever arm's columns are not used; z_p and p_SinI may
 * be NULL); UVIO_HP_POSE_FULL: r = 6, orientation rows first.  R is dense r x r (leading dimension ldr, upper
 * triangle read) in that row order: a mocap covariance couples rotation and translation.
 * rot_handle > 0 names a live quaternion variable of uvio_hp_aux_add_quat as q_ItoS (the dphi block exists only then;
 * q_ItoS is ignored and may be NULL), arm_handle > 0 a live 3-dimensional variable of uvio_hp_aux_add as s (the ds
 * block exists only then and only in FULL mode; p_SinI is ignored).  Both are looked up at replay, value and covariance
 * offset; a handle removed meanwhile refuses the fix (status 3).  z_q and q_ItoS are normalized on entry.
 * Queueing, dropping, the gate (chi2_mult * uvio_hp_chi2_95(r), INFINITY: none), the status codes, the frame that ends
 * in a zero-velocity update and the fatal UVIO_HP_E_NUMERIC are uvio_hp_feed_position's, and the queue is the same
 * one: 256 entries across both kinds.  Replay is merged in ascending time with the UWB messages and the position
 * fixes; at one timestamp the UWB message goes first, then the fixes of both kinds in feed order, each linearized at
 * the state the previous one left.  Consecutive pose fixes of one timestamp run as one device chain with one readback
 * per 8; a change of kind ends a chain.
 * UVIO_HP_E_ARG, before anything is stored: null pointers (z_p in FULL mode among them), a mode that is neither
 * constant, ldr < r, a non-finite t, z_p, read triangle of R or p_SinI, a z_q or q_ItoS that is not finite or whose norm
 * lies outside [0.5, 2], a diagonal of R that is not positive, a chi2_mult that is not positive (or NaN), a rot_handle
 * that is dead or not a quaternion variable, an arm_handle that is dead or not an additive 3-vector.
 * UVIO_HP_E_CAPACITY: 256 fixes are already queued. */
int uvio_hp_feed_pose(uvio_hp_t *h, double t, int mode, const double z_q[4], const double *z_p, const double *R, int ldr,
                      const double q_ItoS[4], int rot_handle, const double *p_SinI, int arm_handle, double chi2_mult,
                      int *queued);
/* The pose fixes consumed by the last camera or simulation feed, in processing order, with
 * uvio_hp_get_position_results' conventions and status codes (that call keeps reporting position fixes only). */
int uvio_hp_get_pose_results(uvio_hp_t *h, double *t, double *chi2, int *status, int cap, int *n);

/* ---- feature-sharded MSCKF update across GPUs (BASELINE.json configs 4-5) ----
 * One process per GPU, each with its own handle fed the same measurement stream (the filter state is
 * replicated).  Inside UpdaterMSCKF::update (UpdaterMSCKF.cpp:58-295) the selected features are split into
 * contiguous chunks balanced by stacked rows (uvio_hp_shard_partition); each rank triangulates, linearizes,
 * nullspace-projects and chi2-gates its own chunk and forms its Gram block [H r]^T [H r]; the blocks are
 * summed across ranks (ncclAllReduce on the library's stream, or a host callback), and every rank applies
 * the same information-form update (the compressed update, UpdaterHelper.cpp:456-487 +
 * StateHelper::EKFUpdate, depends on the stacked rows only through that sum).  Updates with fewer than
 * min_features features run unsharded on every rank.  Every rank must make every feed call. */
/* In-place sum of count doubles (host memory) over all ranks; returns 0 on success. */
typedef int (*uvio_hp_allreduce_fn)(double *buf, size_t count, void *user);
/* ncclGetUniqueId: rank 0 creates it, the caller distributes the 128 bytes to every rank */
int uvio_hp_shard_unique_id(uint8_t id[128]);
/* RCCL communicator over the ranks (ncclCommInitRank: collective, every rank calls it) */
int uvio_hp_shard_init_rccl(uvio_hp_t *h, int rank, int world, const uint8_t id[128], int min_features);
/* host all-reduce callback instead of RCCL (e.g. a gloo process group; ranks may share one GPU) */
int uvio_hp_shard_init_host(uvio_hp_t *h, int rank, int world, uvio_hp_allreduce_fn fn, void *user,
                            int min_features);
/* the partition the update uses: rows[i] = stacked rows of feature i (2 m_f - 3); bounds (world + 1
 * ints) receives the contiguous ranges [bounds[r], bounds[r+1]) balanced by their row sums. */
int uvio_hp_shard_partition(const int *rows, int n, int world, int *bounds);

/* ---- inner (kernel-level) boundary used by parity tests ---- */
/* per-feature results of the last UpdaterMSCKF::update: feature id, triangulated p_FinG (3 per
 * feature), status (0 accepted, 1 triangulation/refinement failed, 3 chi2 rejected) and chi2 */
int uvio_hp_debug_last_msckf(uvio_hp_t *h, uint64_t *ids, double *pG, int *status, double *chi2, int cap, int *n);
/* the correction dx = K res of the last UpdaterMSCKF::update, indexed by covariance id (*n = its length, the
 * covariance dimension at that update; zeros when no feature was accepted; *n = 0 before the first update).  The
 * update reads dx back anyway; this is what a test compares in units of the prior standard deviations, which the
 * updated state, stored in double precision, cannot show.  UVIO_HP_E_CAPACITY when cap < *n. */
int uvio_hp_debug_last_msckf_dx(uvio_hp_t *h, double *dx, int cap, int *n);
/* per-feature results of every updater call of the last camera frame, in call order: kind (0
 * UpdaterMSCKF::update, 1 UpdaterSLAM::update, 2 UpdaterSLAM::delayed_init), feature id, p_FinG (MSCKF:
 * triangulated; delayed init: triangulated before the landmark's initialization; SLAM update: 0),
 * status (0 accepted, 1 triangulation/refinement failed or too few measurements, 3 chi2 rejected) and
 * chi2 (delayed init: StateHelper::initialize's test, StateHelper.cpp:451-470).  The lock-step tests
 * hand these to the oracle's rounding-tie witness (oracle/src/flip.h). */
int uvio_hp_debug_frame_feats(uvio_hp_t *h, int *kind, uint64_t *ids, double *pG, int *status, double *chi2, int cap,
                              int *n);
/* StateHelper::EKFUpdate (StateHelper.cpp:116) on a standalone covariance: P (N x N, row-major,
 * in/out, host memory), H (r x n, row-major) whose column j maps to covariance index H_index[j]
 * (the H_order blocks flattened), residual (r), isotropic noise sigma2.  dx_out (N) receives K*res.
 * The update runs on the device (same kernels as the manager).
 * Limits: r <= 255 rows (the factor panel holds the r rows of S and the residual row) and n <= 1215 columns
 * (16 rows of P[:, H_index] staged in LDS); beyond either the call returns UVIO_HP_E_CAPACITY and touches
 * nothing.  UVIO_HP_E_NUMERIC: the updated covariance has a negative diagonal entry (where the
 * reference exits; P and dx_out hold the update all the same). */
int uvio_hp_ekf_update(double *P, int N, const int *H_index, int n, const double *H, int r,
                       const double *res, double sigma2, double *dx_out);
/* StateHelper::EKFUpdate (StateHelper.cpp:116-197) with a dense noise matrix on a standalone covariance, behind
 * the chi2 gate of UpdaterUWB.cpp:67-79: uvio_hp_ekf_update's arguments and limits with R (r x r, leading
 * dimension ldr, upper triangle read) in place of sigma2, and the gate of uvio_hp_measurement_update (the same
 * three kernels).  *chi2 and *applied are written when the call returns 0.  Not applied: P comes back unchanged
 * and dx_out is zeros.  UVIO_HP_E_ARG also for ldr < r, a chi2_thr that is not positive, non-finite inputs, and an
 * S that is not positive definite (uvio_hp_last_error(NULL) says so). */
int uvio_hp_ekf_update_r(double *P, int N, const int *H_index, int n, const double *H, int r, const double *res,
                         const double *R, int ldr, double chi2_thr, double *dx_out, double *chi2, int *applied);
/* The three kernels of the uvio_hp_aux_* calls on a caller's host covariance, at shapes a test chooses.  P holds
 * at least N + dim (append, init) or N (walk) rows of ld doubles, ld >= that row count; the rows are uploaded with
 * their padding, the kernel runs at leading dimension ld, and the rows come back.
 * _append_p: rows / columns N .. N + dim - 1 <- zeros against [0, N), the prior (dim x dim, ldp, upper triangle
 * read, finite, positive diagonal) mirrored into the block.
 * _init_p: rows / columns N .. N + dim - 1 as uvio_hp_aux_add_from_measurement writes them, H_x (dim x n, ldhx) over
 * the columns H_index (n <= 1215, any order) and H_auxinv = H_aux^-1 (dim x dim, packed) given; res is not read
 * (it only moves the value) and may be NULL.
 * _walk_p: P[i][i] += sigma2 * dt for every component of the ntab blocks [ids[t], ids[t] + dims[t]) (disjoint,
 * dims 1 .. 8; sigma2: the blocks' components concatenated, finite, >= 0; dt finite, >= 0), the product rounded,
 * then the sum.
 * UVIO_HP_E_ARG / UVIO_HP_E_CAPACITY before any device work as for the handle's calls. */
int uvio_hp_aux_append_p(double *P, int N, int ld, int dim, const double *prior, int ldp);
int uvio_hp_aux_init_p(double *P, int N, int ld, int dim, const int *H_index, int n, const double *H_x, int ldhx,
                       const double *H_auxinv, const double *res_unused_or_null, const double *R, int ldr);
int uvio_hp_aux_walk_p(double *P, int N, int ld, int ntab, const int *ids, const int *dims, const double *sigma2,
                       double dt);
/* The three kernels of the buffered position-fix chain (uvio_hp_feed_position) for one fix on a caller's host
 * covariance at a caller's pose: P holds N rows of ld doubles (ld >= N >= 6), uploaded and returned with their
 * padding; the IMU pose's 6 error columns start at imu_id, q[4] = q_GtoI (JPL), p[3] = p_IinG, s[3] the lever arm,
 * whose 3 columns start at aux_id (aux_id < 0: a constant lever arm; the blocks must not overlap).  r, C, z, R, ldr as
 * for uvio_hp_feed_position; chi2_thr positive (INFINITY: no gate).  dx (N) receives the correction, zeros when not
 * applied.  UVIO_HP_E_ARG before any device work for bad arguments, and after it when S is not positive definite (P
 * unchanged); UVIO_HP_E_NUMERIC for a negative diagonal after the update. */
int uvio_hp_debug_position_update_p(double *P, int N, int ld, int imu_id, const double *q, const double *p, int aux_id,
                                    const double *s, int r, const double *C, const double *z, const double *R, int ldr,
                                    double chi2_thr, double *dx, double *chi2, int *applied);
/* The three kernels of the buffered pose-fix chain (uvio_hp_feed_pose) for one fix on a caller's host covariance, with
 * uvio_hp_debug_position_update_p's conventions: q[4] = q_GtoI, p[3] = p_IinG at imu_id, s[3] the lever arm whose 3
 * columns start at arm_id, q_ItoS[4] the mounting rotation whose 3 error columns start at rot_id (either id < 0: a
 * constant; the blocks must not overlap; N >= 6 plus the blocks used).  mode, z_q, z_p, R, ldr as for
 * uvio_hp_feed_pose; an orientation-only fix uses no lever-arm columns. */
int uvio_hp_debug_pose_update_p(double *P, int N, int ld, int imu_id, const double *q, const double *p, int arm_id,
                                const double *s, int rot_id, const double *q_ItoS, int mode, const double *z_q,
                                const double *z_p, const double *R, int ldr, double chi2_thr, double *dx, double *chi2,
                                int *applied);
/* StateHelper::EKFPropagation (StateHelper.cpp:36-114), optionally followed by the clone of the 6-wide IMU pose with
 * its time-offset term (StateHelper.cpp:341-391, 579-616), on a caller's host covariance at shapes a test chooses.  P
 * holds N rows (N + 6 with a clone) of ld doubles, ld >= that row count; the rows go up with their padding, the kernels
 * run at leading dimension ld, the rows come back (N + 6 wide with a clone).  The new block is rows / columns
 * s0 .. s0 + p - 1, or the p distinct indices rows[] (rows != NULL: several variables with a block-row Phi; s0 is
 * not read); iold[q]: the distinct columns Phi (p x q, packed) multiplies; Q (p x p, packed): only its upper triangle
 * is read.  clone != 0: the pose at src0 .. src0 + 5 is cloned to N .. N + 5; dt_id >= 0 adds the time-offset term
 * with column dt_id and dnc[6]; dt_id < 0: no such term (dnc may be NULL).
 * path: UVIO_HP_COV_PATH_AUTO takes what Engine::cov_propagate_clone would take for (N, p, q) -- one k_prop_clone
 * launch when p <= 32, q <= 32 and N p <= 8192, else k_prop_T, k_prop_write and k_clone; _SPLIT forces the latter;
 * _FUSED the former.  *path_ran receives _SPLIT or _FUSED (without a clone always _SPLIT).
 * Before any device work: UVIO_HP_E_ARG for a null pointer, ld below the row count, p or q < 1, an index outside
 * [0, N), a repeated index in rows or iold, rows together with a clone, an unknown path, _FUSED without a clone;
 * UVIO_HP_E_CAPACITY for p > 64 or q > 256 (Engine::cov_propagate's limits) and for _FUSED on a shape k_prop_clone
 * does not take. */
int uvio_hp_debug_cov_propagate_p(double *P, int N, int ld, int s0, int p, const int *rows, const int *iold, int q,
                                  const double *Phi, const double *Q, int clone, int src0, int dt_id, const double *dnc,
                                  int path, int *path_ran);
/* The kernels that copy the covariance into a smaller one, on a caller's host covariance P (N rows of ld doubles,
 * ld >= N >= 1, only read).  op selects:
 *   UVIO_HP_COV_MARGINALIZE        StateHelper::marginalize of [m0, m0 + ms), ms >= 1, m0 + ms <= N; Nn = N - ms
 *   UVIO_HP_COV_MARGINALIZE_MULTI  several of them in one launch: idx[n] the kept indices, strictly ascending; Nn = n
 *   UVIO_HP_COV_COMPACT            P[idx, idx]: idx[n] in [0, N), n <= N, any order; Nn = n
 *   UVIO_HP_COV_MARGINAL_GATHER    uvio_hp_get_marginal_cov's gather: idx[n] in [0, N), any order, repeats allowed,
 *                                  n <= 4096 (else UVIO_HP_E_CAPACITY)
 * out: Nn rows of ld doubles for the first three (uploaded first, so whatever the kernel leaves alone comes back as
 * it was), n x n packed for the gather.  Nn = 0 launches nothing and returns 0.  UVIO_HP_E_ARG before any device
 * work for a null pointer, ld < N, an unknown op or an index outside its range. */
int uvio_hp_debug_cov_gather_p(const double *P, int N, int ld, int op, int m0, int ms, const int *idx, int n,
                               double *out);
/* boost::math::quantile(chi_squared(dof), 0.95), the table every reference updater multiplies its chi2_multipler
 * into (UpdaterMSCKF.cpp:52-55, UpdaterSLAM.cpp:55-58, UpdaterZeroVelocity.cpp:59-62, UpdaterUWB.h:33-36), for
 * dof 1 .. 999; UVIO_HP_E_ARG outside that range. */
int uvio_hp_chi2_95(int dof, double *thr);
/* UpdaterMSCKF.cpp:274-286: measurement_compress_inplace of the stacked [H | res] (m x n) followed by
 * StateHelper::EKFUpdate on the compressed rows, on a standalone covariance (same arguments as
 * uvio_hp_ekf_update).  When m > n the device runs the update in information form on H^T H, H^T res
 * (the quantities the compressed system carries); otherwise it is uvio_hp_ekf_update, with its limits.
 * The information form takes any m and n <= 255 columns (its two factors are n and n + 1 rows of the
 * 256-row panel); a wider H returns UVIO_HP_E_CAPACITY and touches nothing. */
int uvio_hp_msckf_compressed_update(double *P, int N, const int *H_index, int n, const double *H, int m,
                                    const double *res, double sigma2, double *dx_out);
/* UpdaterHelper::measurement_compress_inplace (UpdaterHelper.cpp:456) semantics: A = [H | res]
 * (m x (n+1), row-major) -> the (n+1) x (n+1) upper-triangular R factor of A (rows of the reference's
 * compressed [H|res] up to a per-row sign; the last row holds the residual norm not explained by H).
 * Computed as the Cholesky factor of the Gram matrix: intended for full-column-rank A (the manager's
 * update does not factor the Gram, see uvio_hp_msckf_compressed_update). */
int uvio_hp_compress(const double *A, int m, int n, double *R_out);
/* CamBase::undistort_f (ov_core/src/cam/CamBase.h:89; CamRadtan.h:99 cv::undistortPoints, CamEqui.h:108
 * cv::fisheye::undistortPoints): n pixel points uv (2n floats) -> normalized uvn (2n floats) for model 0
 * (radtan) or 1 (equidistant), cam = fx fy cx cy d0 d1 d2 d3.  Computed on the device; the equidistant
 * points whose float could depend on the last bit of tan are recomputed on the host (ambiguous[i] = 1,
 * may be null), so uvn equals the host libm result for every point. */
int uvio_hp_undistort(int model, const double cam[8], int n, const float *uv, float *uvn, uint8_t *ambiguous);
/* Grider_GRID.h:128 (std::sort(pts_new, Grider_FAST::compare_response)) as the device's FAST cell selection
 * runs it, on caller-given cells: cell c's responses resp[off[c] .. off[c+1]) in cv::FAST's raster order.
 * arrangement (off[ncell] ints) receives each cell's raster indices as libstdc++'s introsort loop leaves them
 * (std::sort's result is their stable order by response); for kmax in 1..64 top (ncell * kmax ints) receives the
 * first min(n, kmax) raster indices of the sorted cell (unused slots untouched).  depth < 0: the reference's
 * 2 lg n depth limit; 0 forces the heap-sort fallback (std::partial_sort(first, last, last)); a depth above 64,
 * more than the kernel's segment stack can hold, is UVIO_HP_E_ARG (checked before any device call).  kmax 0: the
 * whole cell is arranged. */
int uvio_hp_debug_grid_order(const uint8_t *resp, const int *off, int ncell, int kmax, int depth, int *arrangement,
                             int *top);
/* histogram_method 2 (TrackKLT.cpp:56-67, cv::createCLAHE(10.0, Size(8, 8))->apply) as the tracker runs it, on a
 * caller-given 8-bit image of any size w, h >= 9 (rows stride bytes apart): the tracker's own tile-LUT and level-0
 * kernels on a one-level pyramid; out (w * h, packed) receives level 0.  UVIO_HP_E_ARG: null pointers, stride < w,
 * a side below 9; UVIO_HP_E_CAPACITY: a side above 16384. */
int uvio_hp_debug_clahe(const uint8_t *img, int w, int h, int stride, uint8_t *out);
/* One track of uvio_hp_debug_draw_tracks: what display_history reads of it.  (u, v): the track's point in
 * pts_last (centre of the highlight box); hist_n (u, v) pairs from pair hist_off of the call's flat uv array: the
 * feature's uvs of this camera, oldest first (hist_n = 0: the feature is unknown or has no measurement here). */
typedef struct {
  uint64_t id;
  float u, v;
  int highlighted; /* the id is in display_history's highlighted list */
  int n_cams;      /* Feature::uvs.size() (> 1: the stereo colours) */
  int to_delete;   /* Feature::to_delete */
  int hist_off, hist_n;
} uvio_hp_viz_track_t;
/* uvio_hp_get_track_image's renderer on caller-given inputs (the very kernels the getter runs): ncam 8-bit images
 * (imgs[k]: w[k] x h[k], rows strides[k] bytes apart), optional masks (masks == NULL or masks[k] == NULL: none;
 * same size and stride as the image; set where > 127), and per camera counts[k] tracks, concatenated in tracks, in
 * draw order, whose histories lie in uv (n_uv pairs).  out (cap bytes) receives the canvas as
 * uvio_hp_get_track_image returns it; out == NULL only reports the size.  stage_ms (optional, 5 doubles): device
 * milliseconds of the uploads, the base, primitive and compose kernels and the copy out (HIP events).
 * UVIO_HP_E_ARG: null pointers, ncam outside 1..UVIO_HP_MAX_CAMS, a side < 1, stride < w, a negative count, a
 * history outside uv; UVIO_HP_E_CAPACITY: out too small, a side above 16384, or more than 2^31 - 1 primitive
 * pixels. */
int uvio_hp_debug_draw_tracks(int ncam, const uint8_t *const *imgs, const int *w, const int *h, const int *strides,
                              const uint8_t *const *masks, const int *counts, const uvio_hp_viz_track_t *tracks,
                              const float *uv, int n_uv, uint8_t *out, size_t cap, int *width, int *height,
                              double *stage_ms);
/* uvio_hp_get_loop_depth's two images on caller-given inputs through the same path: an 8-bit w x h image (rows
 * stride bytes apart) and n tracks (ids[i], uvd[3 i .. 3 i + 2] = u, v, depth), drawn in ascending id.  depth
 * (w * h uint16_t) and viz (3 * w * h bytes) may each be NULL.  UVIO_HP_E_ARG: null img, a side < 1, stride < w,
 * n < 0, n > 0 without ids / uvd. */
int uvio_hp_debug_loop_depth(const uint8_t *img, int w, int h, int stride, int n, const uint64_t *ids,
                             const double *uvd, uint16_t *depth, uint8_t *viz);
/* device milliseconds of the stages of the handle's last uvio_hp_get_track_image / _device call (HIP events on the
 * library stream): uploads, base, primitives, compose, copy out.  on = 1 switches the event timing on for the
 * following calls (off by default: each timed call records six events), 0 off; ms may be NULL. */
int uvio_hp_debug_track_image_times(uvio_hp_t *h, int on, double ms[5]);
/* the tracker's FAST cells since the handle was created and how many of them had more than 16 candidates
 * (the cells where std::sort's introsort order, not a stable one, decides the selection) */
int uvio_hp_debug_grid_stats(uvio_hp_t *h, uint64_t *cells, uint64_t *introsort_cells);

#ifdef __cplusplus
}
#endif
#endif /* UVIO_HP_H */
