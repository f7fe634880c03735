// Host orchestration of the MI355X hot path.  The host keeps the state *mean* and the variable
// bookkeeping (ids / sizes, like ov_type::Type::_id) and decides what to update; every operation on
// the covariance P runs on the device, where P stays resident for the whole run.
//
// Reference surfaces mirrored: ov_msckf::VioManager (VioManager.cpp:50-651),
// uvio::UVioManager (UVioManager.cpp:26-344), Propagator (Propagator.cpp:33-1015),
// StateHelper (StateHelper.cpp:36-645), UpdaterMSCKF/SLAM (UpdaterMSCKF.cpp, UpdaterSLAM.cpp),
// UpdaterUWB (UpdaterUWB.cpp), FeatureDatabase (FeatureDatabase.cpp).
#pragma once
#include <chrono>
#include <atomic>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <unordered_map>
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "hp_common.h"
#include "fast_prop.h"
#include "hprof.h"
#include "imu_math.h"
#include "kernels.h"
#include "pool.h"
#include "tracker.h"

namespace uvhp {

// V_AUX: a caller-defined additive vector (uvio_hp_aux_add), updated like V_VEC
// V_AUX_QUAT: a caller-defined JPL quaternion (uvio_hp_aux_add_quat), updated like V_QUAT
enum VKind { V_IMU = 0, V_VEC = 1, V_QUAT = 2, V_POSE = 3, V_LANDMARK = 4, V_ANCHOR = 5, V_AUX = 6, V_AUX_QUAT = 7 };

// ov_type::Type bookkeeping + value / first estimate
struct Var {
  VKind kind;
  int id = -1, size = 0, vlen = 0;
  double val[16] = {0}, fej[16] = {0};
  // landmark
  size_t featid = 0;
  int rep = 0, anchor_cam = -1, unique_cam = -1, fail_count = 0;
  double anchor_time = -1;
  bool should_marg = false;
  // ANCHORED_INVERSE_DEPTH_SINGLE: the anchor bearing p / z kept beside the one-dimensional state (Landmark.h:67-70);
  // the state vector does not carry it
  double uvn0[3] = {0, 0, 0}, uvn0_fej[3] = {0, 0, 0};
  // uwb anchor
  uint64_t anchor_id = 0;
  bool fixed = false;
  Var(VKind k, int sz, int vl) : kind(k), size(sz), vlen(vl) {}
  void update(const double *dx);  // Type::update family (JPLQuat.h:114, IMU.h:78, Vec.h:55, ...)
  void xyz(bool fej_, double *out) const;          // Landmark::get_xyz (Landmark.cpp:26)
  void set_xyz(const double *p, bool fej_);        // Landmark::set_from_xyz (Landmark.cpp:65)
};
using VarP = std::shared_ptr<Var>;

// One camera's measurements of a feature (Feature::uvs / uvs_norm / timestamps of that camera,
// Feature.h:39-96), stored together
struct FeatMeas {
  float u, v, un, vn;
  double t;
};
// One camera's measurements in time order.  Trimming the oldest ones (FeatureDatabase::cleanup_measurements,
// every frame, over every feature of the database) only advances a start offset -- the storage is compacted
// once the dead prefix outgrows the live part -- so the per-frame cleanup touches no measurement data.
struct MeasList {
  std::vector<FeatMeas> v;
  size_t b = 0;         // first live entry
  bool sorted = true;   // live entries in non-decreasing time (every in-order stream); the time searches
                        // (contains / drop_through) fall back to the reference's linear scans otherwise
  double tf = 0, tl = 0;  // times of the first and the last live entry (valid when not empty): the selection
                          // scans over every feature decide from these without touching the storage
  using iterator = std::vector<FeatMeas>::iterator;
  using const_iterator = std::vector<FeatMeas>::const_iterator;
  size_t size() const { return v.size() - b; }
  bool empty() const { return v.size() == b; }
  FeatMeas &operator[](size_t i) { return v[b + i]; }
  const FeatMeas &operator[](size_t i) const { return v[b + i]; }
  FeatMeas &back() { return v.back(); }
  const FeatMeas &back() const { return v.back(); }
  const FeatMeas &front() const { return v[b]; }
  iterator begin() { return v.begin() + (std::ptrdiff_t)b; }
  iterator end() { return v.end(); }
  const_iterator begin() const { return v.begin() + (std::ptrdiff_t)b; }
  const_iterator end() const { return v.end(); }
  double last_t() const { return tl; }
  void push_back(const FeatMeas &x) {
    if (v.size() == b)
      tf = x.t;
    else if (x.t < tl)
      sorted = false;
    v.push_back(x);
    tl = x.t;
  }
  // a live entry at time t (FeatureDatabase::features_containing's std::find, FeatureDatabase.cpp:169-208)
  bool contains(double t) const {
    if (sorted) {
      if (empty() || t < tf || t > tl) return false;
      if (t == tf || t == tl) return true;
      auto it = std::lower_bound(begin(), end(), t, [](const FeatMeas &x, double tt) { return x.t < tt; });
      return it != end() && it->t == t;
    }
    for (auto it = begin(); it != end(); ++it)
      if (it->t == t) return true;
    return false;
  }
  // remove every live entry at or before t (Feature::clean_older_measurements, Feature.cpp:85-104)
  void drop_through(double t) {
    if (sorted) {
      auto it = std::upper_bound(begin(), end(), t, [](double tt, const FeatMeas &x) { return tt < x.t; });
      drop_front((size_t)(it - begin()));
      return;
    }
    size_t w = b;
    for (size_t i = b; i < v.size(); i++)
      if (!(v[i].t <= t)) v[w++] = v[i];
    v.resize(w);
    if (v.size() == b) clear();
    recache();
  }
  void recache() {
    if (v.size() > b) tf = v[b].t, tl = v.back().t;
  }
  void clear() {
    v.clear();
    b = 0;
    sorted = true;
  }
  iterator erase(iterator first, iterator last) {  // (callers may have rewritten entries through iterators)
    auto r = v.erase(first, last);
    recache();
    return r;
  }
  void drop_front(size_t k) {  // remove the k oldest live entries
    if (k == 0) return;
    b += k;
    if (b == v.size()) {
      clear();
    } else if (b > 32 && 2 * b > v.size()) {
      v.erase(v.begin(), v.begin() + (std::ptrdiff_t)b);
      b = 0;
    }
    recache();
  }
  void keep_if_valid(const std::vector<double> &valid);  // keep the entries whose time is in `valid` (sorted)
};
struct CamTrack {
  size_t cam;
  MeasList m;
};
// A feature's per-camera tracks, stored in the feature object (no separate allocation: a scan over every
// feature of the database touches one object per feature), in the reference's iteration order (below)
struct TrackSet {
  CamTrack t[UVIO_HP_MAX_CAMS];
  int n = 0;
  CamTrack *begin() { return t; }
  CamTrack *end() { return t + n; }
  const CamTrack *begin() const { return t; }
  const CamTrack *end() const { return t + n; }
  size_t size() const { return (size_t)n; }
  bool empty() const { return n == 0; }
  CamTrack &front() { return t[0]; }
  CamTrack &insert_front(size_t cam) {
    if (n >= UVIO_HP_MAX_CAMS) throw std::runtime_error("feature observed by more than UVIO_HP_MAX_CAMS cameras");
    // the first unused slot moves to the front: its storage may have been reserved ahead (Engine's feature stock)
    CamTrack spare = std::move(t[n]);
    for (int i = n; i > 0; i--) t[i] = std::move(t[i - 1]);
    t[0] = std::move(spare);
    t[0].cam = cam;
    t[0].m.clear();  // (keeps the capacity)
    n++;
    return t[0];
  }
};
// capacity a new track reserves: one measurement per clone of the window and a few spare (a capacity hint
// only, set from max_clone_size by the engine): the per-frame appends then do not reallocate as they grow
inline std::atomic<int> g_track_reserve{0};

struct Feature {
  size_t featid = 0;
  bool to_delete = false;
  bool held = false;     // read by this frame's update chain: trimmed after the chain, not during it
  size_t dense_idx = 0;  // slot in Engine::dense_
  // Per camera, in the iteration order of the reference's unordered_map<size_t, vector<...>> members:
  // with libstdc++ and at most UVIO_HP_MAX_CAMS small integer keys every key sits in its own bucket and
  // a new key is linked at the list front, so iteration runs in reverse first-insertion order
  // (tests/test_oracle.py pins this) -- a camera's first measurement inserts its track at the front.
  TrackSet tracks;
  int anchor_cam_id = -1;
  double anchor_clone_timestamp = -1;
  double p_FinA[3] = {0, 0, 0}, p_FinG[3] = {0, 0, 0};
  CamTrack &track(size_t cam) {
    for (auto &c : tracks)
      if (c.cam == cam) return c;
    CamTrack &c = tracks.insert_front(cam);
    if (const int r = g_track_reserve.load(std::memory_order_relaxed)) c.m.v.reserve((size_t)r);
    return c;
  }
  const CamTrack *find(size_t cam) const {
    for (auto &c : tracks)
      if (c.cam == cam) return &c;
    return nullptr;
  }
  void clean_old_measurements(const std::vector<double> &valid);  // valid: ascending
  void clean_older_measurements(double t);
  int count() const {
    int c = 0;
    for (auto &p : tracks) c += (int)p.m.size();
    return c;
  }
};
using FeatP = std::shared_ptr<Feature>;

// The feature database's map nodes come from bump-allocated 64 KB slabs (a slab is freed once its last node
// is): nodes inserted one after another sit next to each other, and since a new key of this workload lands
// in an empty bucket, which libstdc++ links at the front of its node list, the map's iteration order is
// mostly reverse insertion order -- the selection's walk over every feature (VioManager.cpp:366-392) then
// reads memory in a descending stream instead of one cache miss per node.  The iteration order itself
// depends only on the keys, the bucket policy and the operation sequence, not on where the nodes live.
class NodeSlabs {
 public:
  static constexpr size_t kSlab = size_t(1) << 16;
  NodeSlabs() = default;
  NodeSlabs(const NodeSlabs &) = delete;
  NodeSlabs &operator=(const NodeSlabs &) = delete;
  ~NodeSlabs() {
    if (cur_) std::free(cur_);
  }
  void *alloc(size_t sz) {
    sz = (sz + 15) & ~size_t(15);
    if (!cur_ || cur_->used + sz > kSlab) next_slab();
    void *p = reinterpret_cast<char *>(cur_) + cur_->used;
    cur_->used += sz;
    cur_->live++;
    return p;
  }
  void release(void *p) {
    Slab *s = reinterpret_cast<Slab *>(reinterpret_cast<uintptr_t>(p) & ~(kSlab - 1));
    if (--s->live == 0 && s != cur_) std::free(s);
  }

 private:
  struct Slab {
    size_t used, live;
  };
  static constexpr size_t kHeader = 64;
  Slab *cur_ = nullptr;
  void next_slab() {
    Slab *old = cur_;
    void *m = std::aligned_alloc(kSlab, kSlab);
    if (!m) throw std::bad_alloc();
    cur_ = static_cast<Slab *>(m);
    cur_->used = kHeader;
    cur_->live = 0;
    if (old && old->live == 0) std::free(old);
  }
};
// single-object allocations (the map's nodes) from the slabs, arrays (the bucket array) from operator new
template <class T>
struct SlabAlloc {
  using value_type = T;
  NodeSlabs *s;
  explicit SlabAlloc(NodeSlabs *s_) : s(s_) {}
  template <class U>
  SlabAlloc(const SlabAlloc<U> &o) : s(o.s) {}
  T *allocate(size_t n) {
    if (n == 1 && sizeof(T) <= 256) return static_cast<T *>(s->alloc(sizeof(T)));
    return std::allocator<T>().allocate(n);
  }
  void deallocate(T *p, size_t n) {
    if (n == 1 && sizeof(T) <= 256)
      s->release(p);
    else
      std::allocator<T>().deallocate(p, n);
  }
  template <class U>
  bool operator==(const SlabAlloc<U> &o) const { return s == o.s; }
  template <class U>
  bool operator!=(const SlabAlloc<U> &o) const { return s != o.s; }
};
// clone time -> slot of a batch's clone table (built in time order): a sorted array searched by bisection
// (add_feature looks up every measurement's clone twice; a std::map node chase per lookup was most of the
// MSCKF batch build at cfg4 / cfg5)
struct SlotTable {
  std::vector<double> t;
  void clear() { t.clear(); }
  void push(double x) { t.push_back(x); }  // ascending
  int find(double x) const {
    auto it = std::lower_bound(t.begin(), t.end(), x);
    return (it != t.end() && *it == x) ? (int)(it - t.begin()) : -1;
  }
  int at(double x) const {
    const int s = find(x);
    if (s < 0) throw std::out_of_range("measurement time is not a clone time");
    return s;
  }
};
using DbMap = std::unordered_map<size_t, FeatP, std::hash<size_t>, std::equal_to<size_t>,
                                 SlabAlloc<std::pair<const size_t, FeatP>>>;

// Feature-sharded MSCKF update across replicas.  Every rank holds the same filter; the
// features of an update are split into contiguous row-balanced chunks, each rank linearizes, gates and
// forms the Gram of its own chunk, the (n+1)^2 information blocks are all-reduced (RCCL on the library's
// stream, or a host callback), and every rank applies the identical information-form update.
struct ShardComm {
  bool enabled = false;
  int rank = 0, world = 1;
  int min_features = 1;              // updates with fewer features run unsharded on every rank
  void *nccl = nullptr;              // ncclComm_t (RCCL)
  uvio_hp_allreduce_fn host_fn = nullptr;
  void *host_user = nullptr;
};

// contiguous chunks of `rows` balanced by their sum: bounds[r] .. bounds[r+1] is rank r's range
void shard_partition(const int *rows, int n, int world, int *bounds);
// RCCL through dlopen (no link-time dependency; reuses the copy PyTorch already loaded, if any)
int rccl_unique_id(uint8_t id[128], std::string *err);
void *rccl_comm_init(int rank, int world, const uint8_t id[128]);
void rccl_allreduce_sum(void *comm, double *buf, size_t count, hipStream_t s);
void rccl_comm_destroy(void *comm);

// Device-resident buffers (allocated once at create, sized from the config).  The handles own their memory;
// the raw pointers beside them are views into `chain` / `chain_host` or into the EKF scratch arrays.
struct DeviceBufs {
  // the streams come first: members die in reverse order, so every buffer and event goes before the stream it was
  // used on.  aux: the information-form prefactor's side stream (Engine::info_prefactor); copy: the staging uploads
  Stream stream, aux, copy;
  int ldp = 0;               // P capacity / leading dimension
  DevBuf<double> P, P2;
  DevBuf<double> T;          // propagation scratch (ldp x 64)
  DevBuf<double> Phi, Q, dnc;
  DevBuf<int> iold;
  // update batch
  int max_feat = 0, max_meas_total = 0, max_vars_total = 0, max_rows = 0, ldh = 0, max_ncol = 0;
  DFeatOut *fout = nullptr;
  DevBuf<double> chi2;
  DevBuf<double> H;          // H_all (max_rows x ldh)
  DevBuf<double> Tall;       // H_all P_can (max_rows x ldh), chi2 gate
  DevBuf<double> chi2S;      // per-feature S of the large chi2 gates (launch_chi2_batch grows it)
  DevBuf<double> partials;
  DevBuf<double> R;          // compressed (ncol x ncol, + global Cholesky scratch)
  DevBuf<double> ekf_M, ekf_W, ekf_S, ekf_y, ekf_M3, ekf_Dinv;  // the arrays ekf's views point at
  EkfScratch ekf{};          // passed by value to the launchers: views only (dx / neg lie in dxneg)
  // pinned mirrors of the results block (inside chain_host, below)
  double *dx_host = nullptr;
  int *neg_host = nullptr;
  DFeatOut *fout_host = nullptr;
  // upload staging ring: small host tables of one launch group are packed into pinned memory and sent
  // with ONE copy (stage / stage_flush); the kernels read the device copy directly
  PinBuf<char> stg_h;
  DevBuf<char> stg_d;
  size_t stg_cap = 0, stg_used = 0, stg_flushed = 0;
  long long stg_epoch = 0;  // ring restarts so far (a reservation must not outlive one: the chain checks)
  // [negative-diagonal count (8 B) | dx (cap + 15) | feature results (max features)], mirrored in pinned
  // memory at neg_host / dx_host / fout_host: an update's dx and its batch's results come back in ONE copy
  double *dxneg = nullptr;
  size_t dx_bytes = 0;  // bytes of [count | dx] (the offset of the feature results)
  // feature sharding: the all-reduced [G upper triangle (max_ncol^2) | accepted features | accepted rows]
  DevBuf<double> shard;
  PinBuf<double> shard_host;  // created by shard_init_host
  DevBuf<int> acc;          // accepted features of the last update batch (gates its P update)
  // information-form prefactor on a side stream (Engine::info_prefactor): P_II's factor and V while the
  // feature group runs; its column map in a dedicated device buffer (pinned mirror), the run it belongs to
  Event ev_aux_in, ev_aux_out;
  // staging uploads run on their own stream (the DMA transfer overlaps the kernels already queued on `stream`,
  // which waits on ev_copy before its next launch)
  Event ev_copy;
  // the prefactor's column maps: kPreSlots pinned / device slots used in turn, each freed by its copy's event
  // (a slot is reused kPreSlots prefactors later, so the host never waits on the one just enqueued)
  static constexpr int kPreSlots = 8;
  DevBuf<int> hidx_pre;
  PinBuf<int> hidx_pre_h;
  Event ev_pre[kPreSlots];
  int pre_slot = 0;
  std::vector<int> pre_hidx;  // columns of the pending prefactor (empty: none)
  int pre_N = -1;
  long long pre_epoch = -1;  // Engine::p_epoch_ when the prefactor was enqueued
  // The update chain (Engine::update_frame): per update one region of chain_stride doubles; a delayed-initialization
  // candidate's is [dx (N) | chi2, accepted | init residual (3) | accepted, negative diagonals].  chain_k regions,
  // as many as the covariance has room for updates (alloc_device).
  // The chain's per-update regions sit right in front of dxneg (region r at dxneg - (r + 1) stride), and
  // chain_host mirrors [regions | dx block | fout] in pinned memory, so the chain's regions and every batch's
  // per-feature results come back in ONE copy (chain_results_copy)
  DevBuf<char> chain;  // the allocations: [chain_k regions][dx block][fout]
  PinBuf<char> chain_host;
  int chain_k = 0;
  size_t chain_stride = 0;
  double *region_dev(int r) const { return dxneg - (size_t)(r + 1) * chain_stride; }
  const double *region_host(int r) const { return (const double *)neg_host - (size_t)(r + 1) * chain_stride; }
  int fout_cap = 0;            // per-feature result slots in fout / fout_host (one frame chain's batches)
  DevBuf<char> frame;          // the frame chain's device state: clone / camera tables, pose values, mirror
  size_t frame_bytes = 0;
  // the measurement chains (Engine::run_mchain: the UWB ranges of one message, the position fixes of one
  // timestamp): per step a region (kernels.h DChainRegion, then dx) of mchain_stride doubles in raw device bytes
  // (chain_region types them), the pinned mirror of all regions, and one DChainRow per step.  Either chain ends in
  // its own readback before the other can start, so both use the same kChainMaxSteps slots.
  DevBuf<unsigned char> mchain_reg;
  PinBuf<double> mchain_host;
  size_t mchain_stride = 0;
  DevBuf<DChainRow> mchain_row;
  // Engine::marginal_cov: the gathered m x m block and its pinned mirror (both grow on demand)
  DevBuf<double> marg;
  PinBuf<double> marg_host;
  // IMU-rate odometry (engine_odom.cpp): the 15 x 15 IMU marginal of a published snapshot is gathered into one of
  // two device slots and copied to the matching pinned slot behind the frame's last P write; the slot's event
  // tells a query that its copy has landed.  odom_idx: the IMU's 15 covariance indices.
  static constexpr int kOdomSlot = 15 * 15;
  DevBuf<int> odom_idx;
  DevBuf<double> odom_dev;
  PinBuf<double> odom_host;
  Event ev_odom[2];
};

// The renderer of the image products (engine_viz.cpp): TrackBase::display_history's canvas from device images, host
// masks and tracks.  Its buffers (canvas, priority plane, primitive table, masks and their pinned mirrors) are made
// on the first call and grow on demand; a call returns with its output complete, so nothing is in flight when they
// are replaced.  Nothing here is touched by a feed.
struct VizCamIn {
  const uint8_t *img;    // device, rows `stride` bytes apart
  int w, h, stride;
  const uint8_t *mask;   // host, rows `mask_stride` bytes apart, or null
  int mask_stride;
};
class VizRenderer {
 public:
  // The primitive table of display_history (draw order) for ncam cameras: counts[k] tracks of camera k, concatenated
  // in tracks, histories in uv.  Returns the number of primitive pixels, -1 if it exceeds an int
  static long long build_tracks(int ncam, const VizCamIn *cams, const int *counts, const uvio_hp_viz_track_t *tracks,
                                const float *uv, std::vector<DVizPrim> &prims);
  // the filled squares of publish_loopclosure_information (camera slot 0) and, if depth is given, its 16-bit map
  static long long build_depth(int w, int h, int n, const uint64_t *ids, const double *uvd, std::vector<DVizPrim> &prims,
                               uint16_t *depth);
  // base + primitives + compose on s, then the canvas (3 * ch * ncam * cw bytes) into out_host, or rendered straight
  // into out_dev; waits for s
  void render(hipStream_t s, int ncam, const VizCamIn *cams, const std::vector<DVizPrim> &prims, long long npix,
              uint8_t *out_host, uint8_t *out_dev);
  static void cell(int ncam, const VizCamIn *cams, int *cw, int *ch);
  bool timing = false;
  double ms[5] = {0, 0, 0, 0, 0};  // uploads, base, primitives, compose, copy out of the last timed call

 private:
  struct TimedEvent : HipHandle<hipEvent_t, hipEventDestroy> {
    static TimedEvent create() {
      TimedEvent e;
      HP_HIP(hipEventCreate(&e.h_));
      return e;
    }
  };
  DevBuf<uint8_t> canvas_, d_mask_;
  DevBuf<unsigned long long> plane_;
  DevBuf<DVizPrim> d_prims_;
  PinBuf<DVizPrim> h_prims_;
  PinBuf<uint8_t> h_mask_, h_out_;
  TimedEvent ev_[6];
};

// the per-feature measurement / variable tables of one feature in the reference iteration order (engine_update.cpp)
class Engine;
void add_feature(Engine *, const FeatP &f, int mode, int rep, const uvio_hp_options_t &o, const std::vector<DCam> &cams,
                 const SlotTable &slot_of_time, const std::vector<DClone> &clones, std::vector<DFeat> &feats,
                 std::vector<DMeas> &meas, std::vector<DVar> &vars, int &rows, const Var *landmark, int landmark_canon);
// algorithmic FP64 FLOPs / bytes of one EKFUpdate (engine_state.cpp)
double ekf_flops(double N, double n, double r);
double ekf_bytes(double N, double n, double r);
// a caller's H (r x n, ld ldh), res (r) and the upper triangle of R (r x r, ld ldr) hold finite numbers only
bool ekf_R_inputs_finite(const double *H, int ldh, int r, int n, const double *res, const double *R, int ldr);
// the upper triangle of a caller's d x d matrix (ld) is finite (and, with pos_diag, its diagonal positive)
bool aux_upper_ok(const double *A, int ld, int d, bool pos_diag);
// a finite quaternion whose norm lies in [0.5, 2], normalized into out
bool unit_quat_ok(const double *q, double *out);
// inv (d x d packed) <- A^-1 (d x d, ld lda) by Gauss-Jordan with partial pivoting; false when an entry is not
// finite or a pivot is not above d * 2^-52 * max |A| (singular)
bool aux_inverse(const double *A, int lda, int d, double *inv);

class Engine {
 public:
  explicit Engine(const uvio_hp_options_t &o, int device);
  ~Engine();

  void initialize_with_gt(const double x[17]);
  void feed_imu(double t, const double wm[3], const double am[3]);
  int feed_simulation(double t, int ncam, const int *cam_ids, const int *counts, const uint64_t *ids, const float *uv);
  int feed_camera(double t, int ncam, const int *cam_ids, const uint8_t *const *imgs, const int *strides,
                  const uint8_t *const *masks, bool device_imgs);
  int feed_uwb(double t, int n, const uint64_t *ids, const double *ranges);
  // uvio_hp_feed_position: one position fix into past_fix_, replayed inside the next frame (after_tracking)
  int feed_position(double t, int r, const double *C, const double *z, const double *R, int ldr, const double *p_SinI,
                    int aux_handle, double chi2_mult, int *queued);
  // the fixes the last camera / simulation feed consumed, in processing order
  struct FixResult {
    double t, chi2;
    int status;  // 0 applied, 1 gated, 2 dropped, 3 refused
  };
  const std::vector<FixResult> &position_results() const { return fix_results_; }
  // uvio_hp_feed_pose: one pose fix into the same queue (past_fix_), replayed in feed order with the position fixes
  int feed_pose(double t, int mode, const double *z_q, const double *z_p, const double *R, int ldr, const double *q_ItoS,
                int rot_handle, const double *p_SinI, int arm_handle, double chi2_mult, int *queued);
  const std::vector<FixResult> &pose_results() const { return pose_results_; }
  Tracker *tracker() { return tracker_.get(); }
  int init_anchors(int n, const uvio_hp_anchor_t *a);
  // HIP's current device is per host thread: every C-ABI entry binds the engine's device first, so a handle
  // created for GPU k may be driven from any thread
  int device() const { return device_; }

  // getters
  bool initialized() const { return is_initialized_; }
  double timestamp() const { return timestamp_; }
  const Var &imu() const { return *imu_; }
  int cov_dim() const { return N_; }
  void get_cov(double *out, int ld);
  int state_vector(double *out, int cap, int *meta, int meta_cap, int *nvars, bool fej = false);
  uvio_hp_timing_t timing() const { return timing_; }
  std::vector<double> clone_times() const;

  // live kernel timing of the roofline classes (kprof.h)
  // period 0: off; k: the camera frames whose index is a multiple of k are timed (events cost host time)
  void set_kernel_timing(int period) {
    ktime_period_ = period;
    kprof_.on = period > 0 && frames_ % period == 0;
  }
  void kernel_stats(bool flush, uvio_hp_kstat_t *out, int cap, int *n);

  // feature sharding
  void shard_init_rccl(int rank, int world, const uint8_t id[128], int min_features);
  void shard_init_host(int rank, int world, uvio_hp_allreduce_fn fn, void *user, int min_features);

  // standalone kernel-level entry points (parity tests)
  // ekf_update_standalone's direct form with a dense R and a chi2 gate (launch_ekf_update_R)
  static int ekf_update_R_standalone(double *P, int N, const int *H_index, int n, const double *H, int r,
                                     const double *res, const double *R, int ldr, double chi2_thr, double *dx_out,
                                     double *chi2, int *applied);
  static int ekf_update_standalone(double *P, int N, const int *H_index, int n, const double *H, int r, const double *res,
                                   double sigma2, double *dx_out, bool compress = false);
  static int compress_standalone(const double *A, int m, int n, double *R_out);
  static int undistort_standalone(int model, const double cam[8], int n, const float *uv, float *uvn, uint8_t *amb);
  static int grid_order_standalone(const uint8_t *resp, const int *off, int ncell, int kmax, int depth,
                                   int *arrangement, int *top);
  static int clahe_standalone(const uint8_t *img, int w, int h, int stride, uint8_t *out);
  // the aux-state kernels on a caller's host covariance (uvio_hp_aux_append_p / _init_p / _walk_p)
  static int aux_append_standalone(double *P, int N, int ld, int dim, const double *prior, int ldp);
  static int aux_init_standalone(double *P, int N, int ld, int dim, const int *H_index, int n, const double *H_x,
                                 int ldhx, const double *H_auxinv, const double *R, int ldr);
  static int aux_walk_standalone(double *P, int N, int ld, int ntab, const int *ids, const int *dims,
                                 const double *sigma2, double dt);
  // the covariance bookkeeping kernels on a caller's host covariance (uvio_hp_debug_cov_propagate_p / _cov_gather_p)
  static int cov_propagate_standalone(double *P, int N, int ld, int s0, int p, const int *rows, const int *iold, int q,
                                      const double *Phi, const double *Q, int clone, int src0, int dt_id,
                                      const double *dnc, int path, int *path_ran);
  static int cov_gather_standalone(const double *P, int N, int ld, int op, int m0, int ms, const int *idx, int n,
                                   double *out);
  // the three kernels of the position-fix chain on a caller's host covariance (uvio_hp_debug_position_update_p)
  static int position_update_standalone(double *P, int N, int ld, int imu_id, const double *q, const double *p,
                                        int aux_id, const double *s, int r, const double *C, const double *z,
                                        const double *R, int ldr, double chi2_thr, double *dx, double *chi2,
                                        int *applied);
  // the three kernels of the pose-fix chain on a caller's host covariance (uvio_hp_debug_pose_update_p)
  static int pose_update_standalone(double *P, int N, int ld, int imu_id, const double *q, const double *p, int arm_id,
                                    const double *s, int rot_id, const double *q_ItoS, int mode, const double *z_q,
                                    const double *z_p, const double *R, int ldr, double chi2_thr, double *dx,
                                    double *chi2, int *applied);

 private:
  uvio_hp_options_t o_;
  int device_;
  DeviceBufs d_;
  // ---- state (host mean + bookkeeping) ----
  double timestamp_ = -1;
  VarP imu_, calib_dt_, dw_, da_, tg_, qg_, qa_, p_IinU_;
  std::map<double, VarP> clones_;
  std::unordered_map<size_t, VarP> slam_;
  std::unordered_map<size_t, VarP> calib_pose_, calib_intr_;
  std::unordered_map<size_t, VarP> anchors_;
  CamParams cams_[UVIO_HP_MAX_CAMS];
  std::vector<VarP> vars_;
  int N_ = 0;
  // bumped by every write of P (propagation, clone, marginalization, EKF updates, initialization, uploads):
  // a side-stream prefactor is only used when P is unchanged since it was enqueued
  long long p_epoch_ = 0;
  double early_prop_s_ = 0.0;  // host time of a propagation run inside the tracker's wait (feed_camera)
  // ---- propagator ----
  std::mutex imu_mtx_;
  std::vector<ImuSample> imu_data_;
  bool have_last_prop_time_offset_ = false;
  double last_prop_time_offset_ = 0;
  // ---- KLT front-end (created on the first camera feed) ----
  std::unique_ptr<Tracker> tracker_;
  // ---- feature database (TrackSIM's / TrackKLT's) ----
  NodeSlabs db_nodes_;  // (declared before db_: it outlives the map's nodes)
  DbMap db_{SlabAlloc<std::pair<const size_t, FeatP>>(&db_nodes_)};
  // every feature of db_ in one contiguous array (order unrelated to db_'s; Feature::dense_idx is the slot)
  // for the walks whose outcome does not depend on the order (the per-frame measurement cleanup), which then
  // need not chase the hash map's nodes; db_insert / db_erase keep the two in step
  std::vector<Feature *> dense_;
  using DbIt = DbMap::iterator;
  DbIt db_insert(size_t id, const FeatP &f) {
    f->dense_idx = dense_.size();
    dense_.push_back(f.get());
    return db_.emplace(id, f).first;
  }
  DbIt db_erase(DbIt it) {
    const size_t i = it->second->dense_idx;
    dense_[i] = dense_.back();
    dense_[i]->dense_idx = i;
    dense_.pop_back();
    return db_.erase(it);
  }
  size_t currid_;
  // default-constructed features made while the host waits for the device chain (refill_feature_stock), so
  // that a feed's inserts -- sequential, in observation order -- do not allocate and clear each new object
  std::vector<FeatP> feat_stock_;
  size_t stock_target_ = 0;  // 1.5 x the last feed's new features
  FeatP new_feature(size_t id) {
    FeatP f;
    if (!feat_stock_.empty()) {
      f = std::move(feat_stock_.back());
      feat_stock_.pop_back();
    } else {
      f = std::make_shared<Feature>();
    }
    f->featid = id;
    return f;
  }
  // each stocked feature also gets the storage of its first track reserved (every new feature has one; the
  // feed's first append to it then does not allocate; reserving all cameras' tracks cost more than it saved
  // at cfg5, where a feature is seen by ~2.6 of 4 cameras)
  void refill_feature_stock() {
    const int r = g_track_reserve.load(std::memory_order_relaxed);
    while (feat_stock_.size() < stock_target_) {
      FeatP f = std::make_shared<Feature>();
      if (r > 0) f->tracks.t[0].m.v.reserve((size_t)r);
      feat_stock_.push_back(std::move(f));
    }
  }
  // ---- manager ----
  bool is_initialized_ = false;
  // VioManager::thread_init_success (VioManager.h:226): the initializer succeeded on an earlier frame; the
  // manager reports initialized only on the next camera frame (VioManagerHelper.cpp:91-93, 187)
  bool init_success_ = false;
  // inside feed_camera (the update chain then runs the tracker's next detection ahead, Tracker::predetect);
  // UVIO_HP_NO_PREDETECT=1 turns that off (A/B runs)
  bool camera_frame_ = false, predetect_on_ = true;
  double startup_time_ = -1, distance_ = 0, timelastupdate_ = -1;
  bool anchors_initialized_ = false;
  std::map<double, std::unordered_map<size_t, double>> past_uwb_;
  // the buffered position fixes by time, each time's in feed order (at most kFixQueueMax in all, fix_queued_);
  // after_tracking merges them with past_uwb_ in ascending time
  struct FixMeas {
    int r;
    double C[9], z[3], R[9];  // C: r x 3; R: r x r at leading dimension 3, symmetric
    double s[3];              // the constant lever arm (aux <= 0)
    int aux;                  // aux handle, <= 0: constant lever arm
    double thr;
    // a pose fix (uvio_hp_feed_pose) when pose_r != 0: z holds z_p, s and aux the lever arm, and
    int pose_r = 0;            // 3: orientation only, 6: orientation then position
    double zq[4], qS[4];       // z_q = q_GtoS and the constant q_ItoS (rot <= 0), both unit norm
    int rot = 0;               // aux handle of the mounting rotation, <= 0: constant
    double Rp[36];             // pose_r x pose_r at leading dimension kChainMaxRows, symmetric
  };
  std::map<double, std::vector<FixMeas>> past_fix_;
  int fix_queued_ = 0;
  std::vector<FixResult> fix_results_, pose_results_;
  uvio_hp_timing_t timing_{};
  std::vector<double> chi2_table_;
  ShardComm shard_;
  WorkPool pool_;
  std::vector<FeatP> pending_delete_;  // features handed to an updater this frame (cleanup candidates)
  // host work that update_frame runs while the device executes the chain (set by the caller, cleared by the run)
  std::function<void()> chain_overlap_;
  // FeatureDatabase::cleanup_measurements(t) over the database's features, skipping the held ones if asked
  void cleanup_measurements(double t, bool skip_held);
  void chain_results_copy(int nreg, int fo);
  HostProf hprof_;                     // UVIO_HP_HOST_PROF section timer (debug)
  FILE *timing_csv_ = nullptr;         // record_timing_information (VioManager.cpp:105-122)
  KProf kprof_;                        // live per-class kernel timing (uvio_hp_set_kernel_timing)
  int ktime_period_ = 0;
  long long frames_ = 0;               // camera / simulated frames fed
  void frame_begin() {
    frames_++;
    kprof_.on = ktime_period_ > 0 && frames_ % ktime_period_ == 0;
  }
  void shard_allreduce(double *dev, size_t count);

 public:
  struct FeatDebug {
    size_t id;
    double p_FinG[3];
    int status;
    double chi2;
  };
  // status is the feature kernel's own (2 = refinement failed, which uvio_hp_feat_result_t reports); the debug
  // getters fold it into 1, as the reference's debug output has it (debug_status)
  static int debug_status(int status) { return status == 2 ? 1 : status; }
  std::vector<FeatDebug> last_msckf_;
  // dx of the last UpdaterMSCKF::update (N doubles; zeros when no feature was accepted): uvio_hp_debug_last_msckf_dx
  std::vector<double> last_msckf_dx_;
  std::vector<FeatDebug> last_upd_;  // the last SLAM update / delayed initialization, per feature
  // every updater's per-feature results of the current frame: (kind 0 MSCKF / 1 SLAM update / 2 delayed
  // initialization, result), cleared when the frame's update stage begins (lock-step parity tests)
  std::vector<std::pair<int, FeatDebug>> frame_feats_;

  // updater-level entry points (engine_api.cpp; include/uvio_hp.h "Updater-level boundary")
  enum ApiUpdater { API_MSCKF = 0, API_SLAM = 1, API_DELAYED = 2 };
  int api_set_state(const double *val, const double *fej, int len, const double *P, int N, int ld);
  int api_propagate_and_clone(double t);
  int api_update(int which, int nfeat, const uint64_t *featids, const int *meas_off, const uvio_hp_feat_meas_t *meas,
                 uvio_hp_feat_result_t *out);
  int api_change_anchors();
  int api_marginalize_slam();
  int api_marginalize_old_clone();
  int api_uwb_update_single(uint64_t anchor_id, double range, int *applied);
  // UVioPropagator::propagate (UVioPropagator.cpp:27-115): the state to t without a clone (propagate_uwb)
  int api_propagate(double t);
  // StateHelper::EKFUpdate (StateHelper.cpp:116-197) of a caller's H, residual and dense R over the given blocks of
  // the state, behind the chi2 gate of UpdaterUWB.cpp:67-79 (launch_ekf_update_R); dx moves the mean when applied
  int api_measurement_update(int nvar, const int *ids, const int *sizes, const double *H, int ldh, int r,
                             const double *res, const double *R, int ldr, double chi2_thr, double *chi2, int *applied,
                             double *dx);
  // caller-defined state variables (include/uvio_hp.h uvio_hp_aux_*): appended at N_ on the device
  // (launch_aux_append / launch_aux_init), removed by marginalize
  int api_aux_add(int dim, const double *val, const double *prior, int ld, const double *walk_sigma, int *handle);
  int api_aux_add_quat(const double *q, const double *prior, int ld, const double *walk_sigma, int *handle);
  int api_aux_add_from_measurement(int dim, const double *val0, int nvar, const int *ids, const int *sizes,
                                   const double *H_x, int ldhx, const double *H_aux, int ldha, const double *res,
                                   const double *R, int ldr, const double *walk_sigma, int *handle);
  int api_aux_get(int handle, int *id, int *dim, double *val);
  int api_aux_remove(int handle);
  int api_aux_count(int *n, int *dims_used) const;
  // the reference routine the host was in when the last call failed (error messages)
  const char *stage() const { return stage_; }

  // ---- marginal covariances, the MSCKF features of the frame, IMU-rate odometry (engine_odom.cpp) ----
  // StateHelper::get_marginal_covariance (StateHelper.cpp:226-254): the blocks' rows and columns of P as one dense
  // m x m matrix, gathered on the device
  int marginal_cov(int nvar, const int *ids, const int *sizes, double *out, int ld);
  // VioManager::get_good_features_MSCKF (VioManager.h:123): returns their number (the first cap are written)
  int good_features_msckf(double *xyz_inG, int cap) const;
  void odometry_enable(bool on);
  // Propagator::fast_state_propagate (Propagator.cpp:140-267) from the odometry cache; any thread
  int fast_state_propagate(double t, double *state_plus, double *cov, int *ok);

  // ---- image products (engine_viz.cpp) ----
  // VioManager::get_historical_viz_image: the canvas into out (host, or device memory with device_out); out null
  // only reports the size
  int track_image(uint8_t *out, size_t cap, int *width, int *height, int *overlay, bool device_out);
  int track_history(int cam, uint64_t id, float *uv, int cap, int *n, int *n_cams, int *to_delete) const;
  // the two images of ROS1Visualizer::publish_loopclosure_information for camera 0
  int loop_depth(uint16_t *depth, uint8_t *viz, size_t cap, int *width, int *height, double *t);
  int track_image_times(int on, double *ms);
  static int draw_tracks_standalone(int ncam, const uint8_t *const *imgs, const int *w, const int *h,
                                    const int *strides, const uint8_t *const *masks, const int *counts,
                                    const uvio_hp_viz_track_t *tracks, const float *uv, int n_uv, uint8_t *out,
                                    size_t cap, int *width, int *height, double *stage_ms);
  static int loop_depth_standalone(const uint8_t *img, int w, int h, int stride, int n, const uint64_t *ids,
                                   const double *uvd, uint16_t *depth, uint8_t *viz);

 private:
  std::unique_ptr<VizRenderer> viz_;  // made by the first image call, never by a feed
  const char *stage_ = "";
  std::vector<double> good_feats_;  // good_features_MSCKF (VioManager.cpp:555-570), 3 per feature
  // The odometry cache.  The feed thread marks it stale where the reference calls invalidate_cache()
  // (odom_invalidate) and publishes a snapshot of the filter state at the end of that call (odom_flush); a query
  // adopts the published snapshot before it integrates.  odom_mtx_ guards the cache and the published snapshot;
  // odom_dirty_ and odom_slot_ belong to the feed thread.
  struct OdomSnap {
    bool pending = false;
    int slot = 0;
    double t = 0, t_off = 0, est[16] = {0};
    fastprop::Calib calib{};
  };
  std::atomic<bool> odom_on_{false};
  bool odom_dirty_ = false;
  int odom_slot_ = 0;
  std::mutex odom_mtx_;
  OdomSnap odom_pub_;
  fastprop::Cache odom_cache_;
  bool odom_cache_valid_ = false;
  void odom_invalidate() { odom_dirty_ = true; }
  void odom_flush();

 private:

  // covariance ops (device)
  void alloc_device();
  void upload_P_full(const std::vector<double> &Ph, int N);
  void download_P(std::vector<double> &Ph);
  void cov_propagate(int s0, int p, const std::vector<int> &iold, const std::vector<double> &Phi,
                     const std::vector<double> &Q, const std::vector<int> *rows = nullptr);
  VarP clone_imu_pose(const double *dnc, bool do_dt, const double *staged = nullptr);
  VarP add_clone_var();
  bool cov_propagate_clone(int s0, int p, const std::vector<int> &iold, const std::vector<double> &Phi,
                           const std::vector<double> &Q, bool do_dt, const double *ddnc);
  // The aux registry: handle -> variable and its random-walk variances per second (walk_sigma^2).  aux_walkers_
  // counts the variables with a non-zero density: aux_walk launches nothing while it is 0.
  struct AuxState {
    VarP v;
    double s2[UVIO_HP_AUX_MAX_DIM];
    bool walks;
  };
  std::map<int, AuxState> aux_;
  int aux_next_ = 1, aux_dims_ = 0, aux_walkers_ = 0;
  // the checks every aux_add shares (before any device work); returns walk_sigma^2 in s2
  void aux_check_new(const char *who, int dim, const double *walk_sigma, double *s2) const;
  int aux_register(int dim, const double *val, const double *s2, bool quat = false);
  // P[i][i] += walk_sigma^2 * dt over every walking aux component, one launch (k_aux_walk); called wherever
  // timestamp_ advances by dt
  void aux_walk(double dt);
  void marginalize(const VarP &v);
  // a sequence of marginalize calls as one launch (the same covariance, k_marginalize_multi)
  void marginalize_many(const std::vector<VarP> &ms);
  void check_neg_diag(const char *who);
  void info_prefactor(const std::vector<int> &hidx);
  // joins an information-form prefactor its update did not consume (an early return or an exception in
  // between): the main stream waits for it, so no later P write can overlap its reads of P
  struct PrefactorJoin {
    Engine *e;
    explicit PrefactorJoin(Engine *x) : e(x) {}
    ~PrefactorJoin() {
      if (e->d_.pre_N < 0) return;
      (void)hipStreamWaitEvent(e->d_.stream, e->d_.ev_aux_out, 0);
      e->d_.pre_hidx.clear();
      e->d_.pre_N = -1;
    }
  };
  // a direct EKF update with its own readback (the zero-velocity update): dx goes to the host mean
  void ekf_update_rows(const double *Hdev, int ldh, int r, int n, const std::vector<int> &hidx, const double *resdev,
                       int res_stride, double sigma2);
  void apply_dx(const double *dx);
  // staging (see DeviceBufs): returns the device address the table will have after stage_flush()
  void *stage_bytes(const void *src, size_t bytes);
  // reserve staging space the caller fills in place (host address in *host); same device-address rule.
  // Fill it before the next stage / stage_reserve call (either may flush and recycle the ring).
  void *stage_reserve(size_t bytes, void **host);
  template <class T>
  T *stage(const T *src, size_t n) {
    return (T *)stage_bytes(src, sizeof(T) * n);
  }
  void stage_flush(bool on_main = false);
  // wait for the device (counted in the frame's timing: device_syncs, sync_wait)
  void dev_sync();
  bool propagation_can_precede_tracking(double t) const;
  // dx + negative-diagonal count back to the host (one copy + sync); throws on a negative diagonal
  void read_dx(const char *who);
  void initialize_invertible_host(const VarP &v, const std::vector<std::pair<int, int>> &H_order,
                                  const std::vector<double> &H_R, const std::vector<double> &H_L,
                                  const std::vector<double> &R, const std::vector<double> &res);
  void set_initial_covariance(const std::vector<double> &cov, const std::vector<VarP> &order);

  // start-up from rest (engine_init.cpp): the InertialInitializer's IMU buffer (fed until initialized,
  // VioManager.cpp:180-182), FeatureDatabase::cleanup_measurements, and the initializers
  std::vector<ImuSample> init_imu_;
  void db_cleanup_measurements(double t);
  bool static_initialize(bool wait_for_jerk, double *t_init, std::vector<double> &cov);
  bool try_to_initialize();

  // UpdaterZeroVelocity (UpdaterZeroVelocity.cpp:65-329; VioManager.cpp:160, 186-188, 294-307, 360)
  std::vector<ImuSample> zupt_imu_;
  bool zupt_have_last_off_ = false;
  double zupt_last_off_ = 0.0, last_zupt_state_timestamp_ = 0.0;
  int last_zupt_count_ = 0;
  bool did_zupt_update_ = false, has_moved_since_zupt_ = false;
  // 1: the zero-velocity update was applied (state time moved to t); 0: not
  int zupt_try_update(double t);

  // propagator (host mean + Phi/Qd, device covariance)
  std::vector<ImuSample> select_imu_readings(double t0, double t1);
  void accumulate_phi(const std::vector<ImuSample> &prop, std::vector<double> &Phi, std::vector<double> &Qd, int n);
  void predict_and_compute(const ImuSample &a, const ImuSample &b, double *F, double *Qd, int n);
  void last_w(const std::vector<ImuSample> &prop, double *w);
  std::vector<int> phi_order_ids(int *n);
  int propagate_and_clone(double t);
  int propagate_uwb(double t);

  // updates
  int after_tracking(double t, const std::vector<int> &camids, std::chrono::steady_clock::time_point rT1,
                     int track_syncs = 0, double track_wait = 0.0, bool try_init = false);
  int do_feature_propagate_update(double t, const std::vector<int> &camids, std::chrono::steady_clock::time_point rT2);
  void gram(int m, int ncol, int *nch);
  // VioManager::retriangulate_active_tracks on the device (engine_retri.cpp)
  struct RetriState {
    int cap = 0, obs_cap = 0, slam_cap = 0, cur = 0, nslam = 0;
    DevBuf<unsigned long long> keys[2];
    DevBuf<DRetriEntry> ent[2];
    DevBuf<DRetriObs> d_obs;
    PinBuf<DRetriObs> h_obs;
    DevBuf<DRetriSlam> d_slam;
    PinBuf<DRetriSlam> h_slam;
    DevBuf<double> scratch;
    Event copied;
    bool copy_pending = false, valid = false;
    double time = -1;
    // the frame's job as taken at the reference's point (poses, landmarks, camera models, observations in
    // frame_obs_), run by retri_flush at the next feed's tracking wait or on demand
    bool pend = false, pend_undist = false;
    double pend_t = -1;
    RetriJob pend_job{};
    std::vector<DRetriSlam> pend_sl;
    CamParams pend_cams[UVIO_HP_MAX_CAMS];
  } rt_;
  std::vector<DRetriObs> frame_obs_;  // this frame's observations (simulated feed, or the tracker's last tracks)
  void retri_alloc(int nobs, int nslam);
  void retriangulate_active_tracks(double t, const std::vector<int> &camids);
  void retri_flush();

 public:
  int get_active_tracks(double *t, uint64_t *ids, double *posinG, double *uvd, int *uvd_valid, int cap);
  // a SLAM landmark's position in the global frame: an anchored representation goes through its anchor clone and
  // camera (VioManagerHelper.cpp:422-435)
  void landmark_in_global(const Var &lm, double *p_FinG) const;
  // VioManager::get_features_SLAM (VioManagerHelper.cpp:417): every SLAM landmark, in the order of its variable in
  // the state; returns their number (the first cap are written)
  int get_features_slam(uint64_t *ids, double *xyz_inG, int cap) const;

 private:
  int slam_change_anchors();
  int uwb_update_single(size_t anchor_id, double range);
  // UpdaterUWB::update_single for every range of one UwbData message whose anchor is known, in the message's
  // order, as one device chain with one readback; returns the number of applied updates
  int uwb_update_message(const std::vector<std::pair<size_t, double>> &ranges);
  // The fixes of one timestamp on the current state as device chains of up to kFixMaxChain fixes, one readback each:
  // an aux lever arm's covariance offset and value are resolved here; one FixResult per fix is appended
  void fix_update_chain(double t, const FixMeas *fixes, size_t n);
  // The same for a run of pose fixes (k_pose_rows): an aux lever arm and an aux mounting rotation are resolved here;
  // one FixResult per fix is appended to pose_results_
  void pose_update_chain(double t, const FixMeas *fixes, size_t n);
  // One measurement chain of n <= kChainMaxSteps steps on d_.stream: enqueue(j, prev, row, region) puts step j's
  // three launches there (prev: step j-1's region, null for j = 0).  Then one readback of every region and one
  // wait; returns the pinned regions (step j's at j * d_.mchain_stride doubles: chain_header, then dx).
  template <class F>
  const double *run_mchain(int n, F &&enqueue);
  void marginalize_slam();
  void marginalize_old_clone();
  void db_update(size_t id, double t, size_t cam, float u, float v, float un, float vn);
  double margtimestep() const {
    double t = INFINITY;
    for (auto &c : clones_)
      if (c.first < t) t = c.first;
    return t;
  }

  // batch construction for the per-feature kernel
  struct Batch {
    std::vector<DFeat> feats;
    std::vector<DMeas> meas;
    std::vector<DVar> vars;
    std::vector<DClone> clones;
    std::vector<DCam> cams;
    std::vector<int> hidx;     // canonical column -> covariance id
    // SLAM chunks: the k-step masks of DBatchParams::kmask (two words per feature, then two per 16-row tile)
    std::vector<unsigned long long> kmask;
    const int *hidx_dev = nullptr;  // its staged device copy
    bool finished = false;          // per-feature results read back (finish_batch)
    bool chi2 = true;               // the batch chi2 kernels ran
    std::vector<FeatP> fptrs;
    int n_canon = 0, rows = 0, max_meas = 0, max_nf = 0;
    // large batches write their measurement / variable tables straight into the upload staging
    // (add_features_to_batch); meas / vars then stay empty and these hold the staged tables
    const DMeas *meas_dev = nullptr;
    const DVar *vars_dev = nullptr;
    size_t n_meas_dev = 0, n_vars_dev = 0;
    long long stg_epoch = -1;  // staging ring epoch of the meas / vars reservation
    size_t n_meas() const { return meas_dev ? n_meas_dev : meas.size(); }
    size_t n_vars() const { return vars_dev ? n_vars_dev : vars.size(); }
    SlotTable slot_of_time;
    int fout_off = 0;  // its per-feature results in d_.fout / d_.fout_host start here
  };
  void build_clone_cam_tables(Batch &b, bool include_landmarks);
  void add_feature_to_batch(Batch &b, const FeatP &f, int mode, int rep);
  void add_features_to_batch(Batch &b, const std::vector<FeatP> &fv, size_t lo, size_t hi, int mode, int rep);
  DBatchParams batch_params(const Batch &b, double sigma_pix_sq, double chi2_mult) const;
  // UpdaterMSCKF::update, UpdaterSLAM::update in chunks of slam_chunk features and UpdaterSLAM::delayed_init as
  // one device chain with one host wait (engine_chain.cpp): the frame's three lists, or one updater-level call's
  // list with the other two empty.  `stage` is what stage() names while it runs.
  int update_frame(std::vector<FeatP> &msckf, std::vector<FeatP> &slam_upd, std::vector<FeatP> &delayed,
                   size_t slam_chunk, const char *stage = "update chain");
  struct ChainItem;
  // the chain's replay on the host mean, per kind of item, after the one readback
  void replay_msckf(ChainItem &it);
  void replay_slam(ChainItem &it);
  void replay_delayed(ChainItem &tri, ChainItem &cand, int N0);
  double chain_times_[3] = {0, 0, 0};  // host seconds of the chain's MSCKF / SLAM / delayed-init parts
  // d-wide variables (zeroed landmark slots, d the landmark dimension) at the given covariance offsets leave P in
  // one compaction
  void marginalize_slots(std::vector<int> slots, int d = 3);
  void finish_batch(Batch &b, int mode, std::vector<DFeatOut> &outs);
};

}  // namespace uvhp
