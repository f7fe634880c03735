// Updater-level entry points of the C ABI (include/uvio_hp.h "Updater-level boundary"):
// single updater calls on the engine's current state with caller-provided features, mirroring
// UpdaterMSCKF::update (UpdaterMSCKF.h:68), UpdaterSLAM::update / delayed_init / change_anchors
// (UpdaterSLAM.h:70-87), UpdaterUWB::update_single (UpdaterUWB.h:55), Propagator::propagate_and_clone
// (Propagator.h:110) and StateHelper::marginalize_* (StateHelper.h:224-230).  The same device paths run as
// inside the VioManager frame; only the feature bookkeeping comes from the caller.
#include <unordered_map>

#include "engine.h"

namespace uvhp {

// ov_core::Feature records from the flat arrays: a camera's track is created at its first measurement
// (Feature::track inserts at the front, the map order of the reference's per-camera unordered_maps)
static std::vector<FeatP> make_features(int nfeat, const uint64_t *ids, const int *off, const uvio_hp_feat_meas_t *m,
                                        int ncam) {
  std::vector<FeatP> fv;
  fv.reserve(nfeat);
  for (int i = 0; i < nfeat; i++) {
    if (off[i + 1] < off[i]) throw HpError(UVIO_HP_E_ARG, "meas_off must be non-decreasing");
    auto f = std::make_shared<Feature>();
    f->featid = (size_t)ids[i];
    for (int k = off[i]; k < off[i + 1]; k++) {
      if (m[k].cam < 0 || m[k].cam >= ncam) throw HpError(UVIO_HP_E_ARG, "measurement camera id out of range");
      f->track((size_t)m[k].cam).m.push_back(FeatMeas{m[k].u, m[k].v, m[k].un, m[k].vn, m[k].t});
    }
    fv.push_back(f);
  }
  return fv;
}

int Engine::api_set_state(const double *val, const double *fej, int len, const double *P, int N, int ld) {
  stage_ = "set_state";
  int k = 0;
  for (auto &v : vars_) k += v->vlen;
  if (k != len || N != N_ || ld < N) throw HpError(UVIO_HP_E_ARG, "state snapshot does not match the state layout");
  k = 0;
  for (auto &v : vars_)
    for (int i = 0; i < v->vlen; i++, k++) {
      v->val[i] = val[k];
      v->fej[i] = fej[k];
    }
  if (o_.do_calib_camera_intrinsics)
    for (auto &c : calib_intr_)
      for (int i = 0; i < 8; i++) cams_[c.first].v[i] = c.second->val[i];
  HP_HIP(hipMemcpy2DAsync(d_.P, sizeof(double) * d_.ldp, P, sizeof(double) * ld, sizeof(double) * N, N,
                          hipMemcpyHostToDevice, d_.stream));
  ++p_epoch_;
  dev_sync();
  odom_invalidate();
  odom_flush();
  return 0;
}

int Engine::api_propagate_and_clone(double t) {
  if (!is_initialized_) throw HpError(UVIO_HP_E_STATE, "propagate_and_clone before initialization");
  if (timestamp_ > t) return UVIO_HP_E_ORDER;
  if (timestamp_ == t) return 0;
  return propagate_and_clone(t);
}

int Engine::api_update(int which, int nfeat, const uint64_t *featids, const int *meas_off,
                       const uvio_hp_feat_meas_t *meas, uvio_hp_feat_result_t *out) {
  if (!is_initialized_) throw HpError(UVIO_HP_E_STATE, "updater call before initialization");
  if (nfeat < 0 || (nfeat > 0 && (!featids || !meas_off || !meas || !out))) return UVIO_HP_E_ARG;
  static const char *const routine[3] = {"UpdaterMSCKF::update", "UpdaterSLAM::update", "UpdaterSLAM::delayed_init"};
  if (which < API_MSCKF || which > API_DELAYED) return UVIO_HP_E_ARG;
  stage_ = routine[which];
  const std::vector<FeatP> in = make_features(nfeat, featids, meas_off, meas, o_.num_cameras);
  if (which == API_SLAM)
    for (auto &f : in)
      if (slam_.find(f->featid) == slam_.end()) throw HpError(UVIO_HP_E_ARG, "UpdaterSLAM::update: feature is not a SLAM landmark");
  // The one implementation of the three updaters is the frame's chain (engine_chain.cpp): the caller's list goes
  // into its slot, the other two stay empty.  UpdaterSLAM::update takes its whole list as one batch (the chunks of
  // max_slam_in_update are VioManager's), so the list is a single chunk here.  The chain's other side effects are
  // harmless from this call: it flushes a pending retriangulation (the job was taken at its frame; only the
  // active-track output depends on it) and refills the feature stock (an allocation cache), and chain_times_ /
  // timing_.chain_wait are timing read-outs.  Its errors name the reference routine, as stage() does.
  std::vector<FeatP> lists[3];
  lists[which] = in;
  int rc = 0;
  try {
    rc = update_frame(lists[API_MSCKF], lists[API_SLAM], lists[API_DELAYED], in.size(), routine[which]);
  } catch (const HpError &ex) {
    throw HpError(ex.code, std::string(routine[which]) + ": " + ex.what());
  }
  if (rc) return rc;
  if (which != API_DELAYED) {  // VioManager.cpp:526, 543: after UpdaterMSCKF::update and UpdaterSLAM::update
    odom_invalidate();
    odom_flush();
  }
  const std::vector<FeatDebug> &res = (which == API_MSCKF) ? last_msckf_ : last_upd_;
  std::unordered_map<size_t, const FeatDebug *> by_id;
  for (auto &d : res) by_id[d.id] = &d;
  for (int i = 0; i < nfeat; i++) {
    uvio_hp_feat_result_t &o = out[i];
    o.featid = in[i]->featid;
    o.to_delete = in[i]->to_delete ? 1 : 0;
    auto it = by_id.find(in[i]->featid);
    if (it == by_id.end()) {  // cleaned away before the batch (too few measurements in the clone window)
      o.status = 1;
      o.chi2 = 0.0;
      for (int k = 0; k < 3; k++) o.p_FinG[k] = 0.0;
    } else {
      o.status = it->second->status;
      o.chi2 = it->second->chi2;
      for (int k = 0; k < 3; k++) o.p_FinG[k] = it->second->p_FinG[k];
    }
  }
  return 0;
}

int Engine::api_change_anchors() {
  if (!is_initialized_) throw HpError(UVIO_HP_E_STATE, "change_anchors before initialization");
  return slam_change_anchors();
}

int Engine::api_marginalize_slam() {
  if (!is_initialized_) throw HpError(UVIO_HP_E_STATE, "marginalize_slam before initialization");
  marginalize_slam();
  return 0;
}

int Engine::api_marginalize_old_clone() {
  if (!is_initialized_) throw HpError(UVIO_HP_E_STATE, "marginalize_old_clone before initialization");
  marginalize_old_clone();
  return 0;
}

int Engine::api_uwb_update_single(uint64_t anchor_id, double range, int *applied) {
  if (!is_initialized_) throw HpError(UVIO_HP_E_STATE, "UWB update before initialization");
  const int a = uwb_update_single((size_t)anchor_id, range);
  if (applied) *applied = a;
  return 0;
}

// UVioPropagator::propagate (UVioPropagator.cpp:27-115): Engine::propagate_uwb with its two quirks (the end time
// carries no camera-IMU offset, last_prop_time_offset stays).  No clone, and the odometry cache is left alone, as
// after propagate_and_clone.
int Engine::api_propagate(double t) {
  if (!is_initialized_) throw HpError(UVIO_HP_E_STATE, "propagate before initialization");
  if (!(timestamp_ < t)) return UVIO_HP_E_ORDER;
  return propagate_uwb(t);
}

// StateHelper::EKFUpdate(state, H_order, H, res, R) (StateHelper.cpp:116-197) behind the chi2 test of
// UpdaterUWB.cpp:67-79, for a measurement of the caller's: H_order is the list of covariance blocks.  H with the
// residual as its last column, R's upper triangle and the column map go up as one staged table; the three launches of
// launch_ekf_update_R follow and one readback returns [negative diagonals | dx | chi2, accepted]: one host wait,
// as in ekf_update_rows.  Every refusal but the positive-definiteness one comes before any device work.
int Engine::api_measurement_update(int nvar, const int *ids, const int *sizes, const double *H, int ldh, int r,
                                   const double *res, const double *R, int ldr, double chi2_thr, double *chi2,
                                   int *applied, double *dx) {
  if (!is_initialized_) throw HpError(UVIO_HP_E_STATE, "measurement update before initialization");
  stage_ = "StateHelper::EKFUpdate (measurement_update)";
  if (!chi2 || !applied || nvar < 0 || r < 0) return UVIO_HP_E_ARG;
  if (!(chi2_thr > 0.0)) throw HpError(UVIO_HP_E_ARG, "measurement_update: the chi2 threshold must be positive");
  if (nvar > 0 && (!ids || !sizes)) return UVIO_HP_E_ARG;
  long long nl = 0;
  for (int k = 0; k < nvar; k++) {
    if (sizes[k] < 1 || ids[k] < 0 || (long long)ids[k] + sizes[k] > N_)
      throw HpError(UVIO_HP_E_ARG, "measurement_update: a block lies outside the state");
    nl += sizes[k];
  }
  if (nvar == 0 || r == 0) {
    *chi2 = 0.0;
    *applied = 0;
    if (dx) std::fill(dx, dx + N_, 0.0);
    return 0;
  }
  if (!H || !res || !R) return UVIO_HP_E_ARG;
  if (ldh < nl || ldr < r) throw HpError(UVIO_HP_E_ARG, "measurement_update: leading dimension below the row length");
  if (r > kMaxEkfRows) throw HpError(UVIO_HP_E_CAPACITY, "measurement_update: more than 255 rows");
  if (nl > 1215) throw HpError(UVIO_HP_E_CAPACITY, "measurement_update: more than 1215 columns");
  const int n = (int)nl;
  if (!ekf_R_inputs_finite(H, ldh, r, n, res, R, ldr))
    throw HpError(UVIO_HP_E_ARG, "measurement_update: H, res or the upper triangle of R is not finite");
  const int ldd = n + 1;
  const size_t nH = (size_t)r * ldd, nR = (size_t)r * r;
  const size_t bytes = sizeof(double) * (nH + nR) + sizeof(int) * (size_t)n;
  if ((bytes + 255) / 256 * 256 > d_.stg_cap)
    throw HpError(UVIO_HP_E_CAPACITY, "measurement_update: H does not fit the upload staging ring");
  void *hv = nullptr;
  double *dH = (double *)stage_reserve(bytes, &hv);
  double *hH = (double *)hv, *hR = hH + nH;
  int *hI = (int *)(hR + nR);
  for (int i = 0; i < r; i++) {
    std::memcpy(hH + (size_t)i * ldd, H + (size_t)i * ldh, sizeof(double) * n);
    hH[(size_t)i * ldd + n] = res[i];
    for (int j = 0; j < r; j++) hR[(size_t)i * r + j] = j >= i ? R[(size_t)i * ldr + j] : 0.0;
  }
  for (int k = 0, c = 0; k < nvar; k++)
    for (int i = 0; i < sizes[k]; i++) hI[c++] = ids[k] + i;
  const double *dR = dH + nH;
  const int *dI = (const int *)(dR + nR);
  stage_flush();
  EkfScratch sc = d_.ekf;
  sc.Tall = nullptr;
  sc.kmask_tile = nullptr;
  sc.gate = nullptr;
  sc.chi2_gate = (int *)(sc.dx + N_ + 2);  // behind [chi2, accepted]; the dx block holds cap + 15 doubles
  {
    KScope ks(&kprof_, KC_EKF);
    launch_ekf_update_R(d_.stream, d_.P, d_.ldp, N_, dH, ldd, r, n, dI, dH + n, ldd, dR, r, chi2_thr, sc);
    ++p_epoch_;
  }
  kprof_.credit(KC_EKF, ekf_flops(N_, n, r), ekf_bytes(N_, n, r));
  read_dx("measurement_update");
  const double c2 = d_.dx_host[N_];
  const bool acc = d_.dx_host[N_ + 1] != 0.0;
  *chi2 = c2;
  *applied = acc ? 1 : 0;
  if (!acc) {
    if (dx) std::fill(dx, dx + N_, 0.0);
    if (!std::isfinite(c2))
      throw HpError(UVIO_HP_E_ARG, "measurement_update: S = H P H^T + R is not positive definite; nothing was applied");
    return 0;
  }
  apply_dx(d_.dx_host);
  if (dx) std::memcpy(dx, d_.dx_host, sizeof(double) * N_);
  odom_invalidate();  // as after UpdaterMSCKF::update (VioManager.cpp:526)
  odom_flush();
  return 0;
}

// ---- caller-defined state variables (include/uvio_hp.h uvio_hp_aux_*) ----
// What uvio does for p_IinU and its anchors at start-up through the host (set_initial_covariance,
// initialize_invertible_host: two copies of P) for a caller's variable on a running filter: the new rows and columns
// are written on the device from one staged table, nothing comes back.  Every refusal precedes the device work.
void Engine::aux_check_new(const char *who, int dim, const double *walk_sigma, double *s2) const {
  if (!is_initialized_) throw HpError(UVIO_HP_E_STATE, std::string(who) + " before initialization");
  if (dim < 1 || dim > UVIO_HP_AUX_MAX_DIM) throw HpError(UVIO_HP_E_ARG, std::string(who) + ": dim outside 1 .. 8");
  for (int k = 0; k < dim; k++) {
    const double w = walk_sigma ? walk_sigma[k] : 0.0;
    if (!std::isfinite(w) || w < 0.0)
      throw HpError(UVIO_HP_E_ARG, std::string(who) + ": walk_sigma must be finite and not negative");
    s2[k] = w * w;
  }
  if (aux_dims_ + dim > o_.max_aux_dim || N_ + dim > d_.ldp)
    throw HpError(UVIO_HP_E_CAPACITY, std::string(who) + ": the aux dimensions in use (" + std::to_string(aux_dims_) +
                                          ") plus " + std::to_string(dim) + " exceed max_aux_dim = " +
                                          std::to_string(o_.max_aux_dim));
}

// the variable enters vars_ at offset N_ (its covariance rows / columns are already enqueued)
int Engine::aux_register(int dim, const double *val, const double *s2, bool quat) {
  ++p_epoch_;
  VarP v = quat ? std::make_shared<Var>(V_AUX_QUAT, 3, 4) : std::make_shared<Var>(V_AUX, dim, dim);
  for (int k = 0; k < v->vlen; k++) v->val[k] = v->fej[k] = val[k];
  v->id = N_;
  N_ += dim;
  vars_.push_back(v);
  AuxState a{v, {0}, false};
  for (int k = 0; k < dim; k++) a.s2[k] = s2[k], a.walks = a.walks || s2[k] > 0.0;
  const int handle = aux_next_++;
  aux_[handle] = a;
  aux_dims_ += dim;
  aux_walkers_ += a.walks ? 1 : 0;
  odom_invalidate();
  odom_flush();
  return handle;
}

int Engine::api_aux_add(int dim, const double *val, const double *prior, int ld, const double *walk_sigma, int *handle) {
  stage_ = "aux_add";
  if (!is_initialized_) throw HpError(UVIO_HP_E_STATE, "aux_add before initialization");
  if (!val || !prior || !handle) return UVIO_HP_E_ARG;
  double s2[UVIO_HP_AUX_MAX_DIM];
  aux_check_new("aux_add", dim, walk_sigma, s2);
  if (ld < dim) throw HpError(UVIO_HP_E_ARG, "aux_add: leading dimension below the row length");
  for (int k = 0; k < dim; k++)
    if (!std::isfinite(val[k])) throw HpError(UVIO_HP_E_ARG, "aux_add: val is not finite");
  if (!aux_upper_ok(prior, ld, dim, true))
    throw HpError(UVIO_HP_E_ARG, "aux_add: the upper triangle of prior_cov must be finite with a positive diagonal");
  void *hv = nullptr;
  const double *dpr = (const double *)stage_reserve(sizeof(double) * dim * dim, &hv);
  double *hp = (double *)hv;
  for (int i = 0; i < dim; i++)
    for (int j = 0; j < dim; j++) hp[i * dim + j] = j >= i ? prior[(size_t)i * ld + j] : 0.0;
  stage_flush();
  launch_aux_append(d_.stream, d_.P, d_.ldp, N_, dim, dpr);
  *handle = aux_register(dim, val, s2);
  return 0;
}

// A JPL unit quaternion of the caller's (3 error dimensions, q <- dq(dtheta) (x) q): aux_add's refusals in aux_add's
// order, the same append kernel at dim = 3, the same walk
int Engine::api_aux_add_quat(const double *q, const double *prior, int ld, const double *walk_sigma, int *handle) {
  stage_ = "aux_add_quat";
  if (!is_initialized_) throw HpError(UVIO_HP_E_STATE, "aux_add_quat before initialization");
  if (!q || !prior || !handle) return UVIO_HP_E_ARG;
  double s2[UVIO_HP_AUX_MAX_DIM];
  aux_check_new("aux_add_quat", 3, walk_sigma, s2);
  if (ld < 3) throw HpError(UVIO_HP_E_ARG, "aux_add_quat: leading dimension below the row length");
  double qn[4];
  if (!unit_quat_ok(q, qn)) throw HpError(UVIO_HP_E_ARG, "aux_add_quat: q is not finite or its norm is outside [0.5, 2]");
  if (!aux_upper_ok(prior, ld, 3, true))
    throw HpError(UVIO_HP_E_ARG, "aux_add_quat: the upper triangle of prior_cov must be finite with a positive diagonal");
  void *hv = nullptr;
  const double *dpr = (const double *)stage_reserve(sizeof(double) * 9, &hv);
  double *hp = (double *)hv;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) hp[i * 3 + j] = j >= i ? prior[(size_t)i * ld + j] : 0.0;
  stage_flush();
  launch_aux_append(d_.stream, d_.P, d_.ldp, N_, 3, dpr);
  *handle = aux_register(3, qn, s2, true);
  return 0;
}

int Engine::api_aux_add_from_measurement(int dim, const double *val0, int nvar, const int *ids, const int *sizes,
                                         const double *H_x, int ldhx, const double *H_aux, int ldha, const double *res,
                                         const double *R, int ldr, const double *walk_sigma, int *handle) {
  stage_ = "StateHelper::initialize_invertible (aux_add_from_measurement)";
  const char *who = "aux_add_from_measurement";
  if (!is_initialized_) throw HpError(UVIO_HP_E_STATE, "aux_add_from_measurement before initialization");
  if (!val0 || !H_aux || !res || !R || !handle || nvar < 0 || (nvar > 0 && (!ids || !sizes))) return UVIO_HP_E_ARG;
  double s2[UVIO_HP_AUX_MAX_DIM];
  aux_check_new(who, dim, walk_sigma, s2);
  long long nl = 0;
  for (int k = 0; k < nvar; k++) {
    if (sizes[k] < 1 || ids[k] < 0 || (long long)ids[k] + sizes[k] > N_)
      throw HpError(UVIO_HP_E_ARG, std::string(who) + ": a block lies outside the state");
    nl += sizes[k];
  }
  if (nl > kAuxMaxCols) throw HpError(UVIO_HP_E_CAPACITY, std::string(who) + ": more than 1215 columns");
  const int n = (int)nl;
  if (n > 0 && !H_x) return UVIO_HP_E_ARG;
  if (ldhx < n || ldha < dim || ldr < dim)
    throw HpError(UVIO_HP_E_ARG, std::string(who) + ": leading dimension below the row length");
  bool finite = aux_upper_ok(R, ldr, dim, false);
  for (int i = 0; i < dim && finite; i++) {
    finite = std::isfinite(val0[i]) && std::isfinite(res[i]);
    for (int k = 0; k < n && finite; k++) finite = std::isfinite(H_x[(size_t)i * ldhx + k]);
  }
  if (!finite) throw HpError(UVIO_HP_E_ARG, std::string(who) + ": val0, H_x, res or the upper triangle of R is not finite");
  double Hinv[UVIO_HP_AUX_MAX_DIM * UVIO_HP_AUX_MAX_DIM];
  if (!aux_inverse(H_aux, ldha, dim, Hinv))
    throw HpError(UVIO_HP_E_ARG, std::string(who) + ": H_aux is singular or not finite");
  const size_t nH = (size_t)dim * n, nD = (size_t)dim * dim;
  const size_t bytes = sizeof(double) * (nH + 2 * nD) + sizeof(int) * (size_t)n;
  if ((bytes + 255) / 256 * 256 > d_.stg_cap)
    throw HpError(UVIO_HP_E_CAPACITY, std::string(who) + ": H_x does not fit the upload staging ring");
  // one staged table: [H_x (dim x n) | H_aux^-1 | R's upper triangle | column map]
  void *hv = nullptr;
  const double *dH = (const double *)stage_reserve(bytes, &hv);
  double *hH = (double *)hv, *hD = hH + nH, *hR = hD + nD;
  int *hI = (int *)(hR + nD);
  for (int i = 0; i < dim; i++) {
    if (n > 0) std::memcpy(hH + (size_t)i * n, H_x + (size_t)i * ldhx, sizeof(double) * n);
    for (int j = 0; j < dim; j++) {
      hD[i * dim + j] = Hinv[i * dim + j];
      hR[i * dim + j] = j >= i ? R[(size_t)i * ldr + j] : 0.0;
    }
  }
  for (int k = 0, c = 0; k < nvar; k++)
    for (int i = 0; i < sizes[k]; i++) hI[c++] = ids[k] + i;
  stage_flush();
  // d_.T (ldp x 64, the propagation's scratch) holds Ma (N x dim)
  launch_aux_init(d_.stream, d_.P, d_.ldp, N_, dim, dH, n, n, (const int *)(dH + nH + 2 * nD), dH + nH, dH + nH + nD,
                  d_.T);
  // new_variable->update(H_Linv * res) (StateHelper.cpp:567)
  double val[UVIO_HP_AUX_MAX_DIM];
  for (int a = 0; a < dim; a++) {
    double dx = 0.0;
    for (int b = 0; b < dim; b++) dx += Hinv[a * dim + b] * res[b];
    val[a] = val0[a] + dx;
  }
  *handle = aux_register(dim, val, s2);
  return 0;
}

int Engine::api_aux_get(int handle, int *id, int *dim, double *val) {
  if (!is_initialized_) throw HpError(UVIO_HP_E_STATE, "aux_get before initialization");
  if (!id || !dim) return UVIO_HP_E_ARG;
  auto it = aux_.find(handle);
  if (it == aux_.end()) throw HpError(UVIO_HP_E_ARG, "aux_get: no live aux variable has this handle");
  const Var &v = *it->second.v;
  *id = v.id;
  *dim = v.size;
  if (val) std::memcpy(val, v.val, sizeof(double) * v.vlen);  // a quaternion variable: dim 3, 4 values
  return 0;
}

int Engine::api_aux_remove(int handle) {
  stage_ = "StateHelper::marginalize (aux_remove)";
  if (!is_initialized_) throw HpError(UVIO_HP_E_STATE, "aux_remove before initialization");
  auto it = aux_.find(handle);
  if (it == aux_.end()) throw HpError(UVIO_HP_E_ARG, "aux_remove: no live aux variable has this handle");
  const AuxState a = it->second;
  aux_.erase(it);
  aux_dims_ -= a.v->size;
  aux_walkers_ -= a.walks ? 1 : 0;
  marginalize(a.v);
  odom_invalidate();
  odom_flush();
  return 0;
}

int Engine::api_aux_count(int *n, int *dims_used) const {
  if (n) *n = (int)aux_.size();
  if (dims_used) *dims_used = aux_dims_;
  return 0;
}

}  // namespace uvhp
