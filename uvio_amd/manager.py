"""Python mirror of the reference manager surface (ov_msckf::VioManager / uvio::UVioManager).

Method names follow the reference C++ API (VioManager.h:75-111, UVioManager.h:48-73):
``feed_measurement_imu``, ``feed_measurement_simulation``, ``feed_measurement_uwb``,
``try_to_initialize_uwb_anchors``, ``initialize_with_gt``, ``initialized``, ``get_state`` ...
Every call goes through the C ABI of libuvio_hp.so (include/uvio_hp.h); the estimator state and the
covariance live on the MI355X.  Errors the reference would turn into ``std::exit`` raise here.
"""
import ctypes as C

import numpy as np

from . import _native as N


def load_options(yaml_path=None, **overrides):
    """VioManagerOptions::print_and_load equivalent: defaults, then the YAML keys, then overrides."""
    lib = N.load()
    opts = N.Options()
    N.check(lib.uvio_hp_options_default(C.byref(opts)), what="options_default")
    if yaml_path is not None:
        N.check(lib.uvio_hp_options_load(yaml_path.encode(), C.byref(opts)), what="options_load(%s)" % yaml_path)
    apply_overrides(opts, overrides)
    return opts


def _mask_ptrs(masks, ncam):
    """per-camera u8 masks (None: no mask for that camera) -> (kept arrays, uint8_t*[ncam])"""
    mk = [None if m is None else np.ascontiguousarray(m, dtype=np.uint8) for m in masks]
    ptrs = [C.POINTER(C.c_uint8)() if m is None else m.ctypes.data_as(C.POINTER(C.c_uint8)) for m in mk]
    return mk, (C.POINTER(C.c_uint8) * ncam)(*ptrs)


def apply_overrides(opts, overrides):
    for k, v in overrides.items():
        if not hasattr(opts, k):
            raise KeyError(k)
        setattr(opts, k, v)
    return opts


def shard_unique_id():
    """ncclGetUniqueId (rank 0): 128 bytes to distribute to every rank for enable_feature_sharding."""
    lib = N.load()
    uid = (C.c_uint8 * 128)()
    rc = lib.uvio_hp_shard_unique_id(uid)
    if rc != 0:
        msg = (lib.uvio_hp_last_error(None) or b"").decode()
        raise RuntimeError("shard_unique_id failed: %s %s" % (N.ERRNAMES.get(rc, rc), msg))
    return bytes(uid)


def host_allreduce_callback(group=None):
    """uvio_hp_allreduce_fn over torch.distributed: the library hands a host buffer of doubles, the
    callback sums it in place across the ranks of `group` (default group when None)."""
    import torch
    import torch.distributed as dist

    def _allreduce(buf, count, user):
        try:
            t = torch.from_numpy(np.ctypeslib.as_array(buf, shape=(count,)))
            dist.all_reduce(t, group=group)
            return 0
        except Exception:  # noqa: BLE001
            return 1

    return N.ALLREDUCE_FN(_allreduce)


def shard_partition(rows, world):
    """The feature split the sharded update uses: bounds (world + 1) of contiguous row-balanced chunks."""
    lib = N.load()
    r = np.ascontiguousarray(rows, dtype=np.int32)
    b = np.zeros(world + 1, dtype=np.int32)
    rc = lib.uvio_hp_shard_partition(r.ctypes.data_as(C.POINTER(C.c_int)), len(r), world,
                                     b.ctypes.data_as(C.POINTER(C.c_int)))
    if rc != 0:
        raise RuntimeError("shard_partition failed: %s" % N.ERRNAMES.get(rc, rc))
    return b


def pack_sim_frame(feats):
    """(counts, ids uint64[n], uv float32[n, 2]) of one TrackSIM frame, cameras concatenated."""
    counts = [len(f[0]) for f in feats]
    ids = np.ascontiguousarray(np.concatenate([np.asarray(f[0], dtype=np.uint64) for f in feats]))
    uv = np.ascontiguousarray(np.concatenate([np.asarray(f[1], dtype=np.float32).reshape(-1, 2) for f in feats]))
    return counts, ids, uv


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class VioManager:
    """Handle on one estimator instance (one MI355X device)."""

    _prefix = "uvio_hp_"

    def __init__(self, options, device=0):
        self._lib = self._load()
        self._device = int(device)
        self._h = C.c_void_p()
        rc = self._call("create", C.byref(options), device, C.byref(self._h)) if self._prefix == "uvio_hp_" else \
            self._call("create", C.byref(options), C.byref(self._h))
        if rc != 0:
            why = ""
            if self._prefix == "uvio_hp_":
                msg = self._call("last_error", None)
                why = ": " + msg.decode() if msg else ""
            raise RuntimeError("%screate failed: %s%s" % (self._prefix, N.ERRNAMES.get(rc, rc), why))
        self.options = options

    @classmethod
    def _load(cls):
        return N.load()

    def _call(self, name, *args):
        return getattr(self._lib, self._prefix + name)(*args)

    def _check(self, rc, what):
        if rc != 0:
            msg = ""
            if self._prefix == "uvio_hp_":
                msg = (self._lib.uvio_hp_last_error(self._h) or b"").decode()
            raise RuntimeError("%s failed: %s %s" % (what, N.ERRNAMES.get(rc, rc), msg))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._call("destroy", self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    # ---- feature sharding across ranks (include/uvio_hp.h) ----
    def enable_feature_sharding(self, rank, world, backend="rccl", unique_id=None, group=None, min_features=1):
        """Split every MSCKF update with >= min_features features across `world` replicas of this filter
        (one per rank, all fed the same stream).  backend "rccl": the library all-reduces on its own
        stream over an RCCL communicator (unique_id: the 128 bytes of shard_unique_id() made on rank 0 and
        shared with every rank).  backend "host": the blocks go through torch.distributed.all_reduce on
        `group` (e.g. gloo; ranks may then share one GPU)."""
        if backend == "rccl":
            if unique_id is None or len(unique_id) != 128:
                raise ValueError("rccl backend needs the 128-byte unique id of shard_unique_id()")
            uid = (C.c_uint8 * 128)(*bytearray(unique_id))
            self._check(self._call("shard_init_rccl", self._h, rank, world, uid, min_features), "shard_init_rccl")
        elif backend == "host":
            self._allreduce_cb = host_allreduce_callback(group)  # kept alive with the handle
            fn = C.cast(self._allreduce_cb, C.c_void_p)
            self._check(self._call("shard_init_host", self._h, rank, world, fn, None, min_features),
                        "shard_init_host")
        else:
            raise ValueError("backend must be 'rccl' or 'host'")

    # ---- feeds ----
    def initialize_with_gt(self, imustate17):
        x = np.ascontiguousarray(imustate17, dtype=np.float64)
        assert x.shape == (17,)
        self._check(self._call("initialize_with_gt", self._h, _dp(x)), "initialize_with_gt")

    def feed_measurement_imu(self, t, wm, am):
        w = (C.c_double * 3)(*wm)
        a = (C.c_double * 3)(*am)
        self._check(self._call("feed_imu", self._h, C.c_double(t), w, a), "feed_measurement_imu")

    def feed_measurement_imu_batch(self, t, wm, am):
        """n consecutive feed_measurement_imu calls: t (n,), wm (n,3), am (n,3)."""
        t = np.ascontiguousarray(t, dtype=np.float64)
        wm = np.ascontiguousarray(wm, dtype=np.float64)
        am = np.ascontiguousarray(am, dtype=np.float64)
        n = t.shape[0]
        assert wm.shape == (n, 3) and am.shape == (n, 3)
        if "feed_imu_batch" in N.MISSING:  # an older library under A/B
            for i in range(n):
                self.feed_measurement_imu(float(t[i]), wm[i], am[i])
            return
        self._check(self._call("feed_imu_batch", self._h, n, _dp(t), _dp(wm), _dp(am)), "feed_measurement_imu_batch")

    def feed_measurement_simulation(self, t, camids, feats, allow_uninit=False):
        """feats[i] = (ids uint64[n], uv float32[n,2]) for camera camids[i] (TrackSIM input)."""
        return self.feed_measurement_simulation_packed(t, camids, *pack_sim_frame(feats), allow_uninit=allow_uninit)

    def feed_measurement_simulation_packed(self, t, camids, counts, ids, uv, allow_uninit=False):
        """feed_measurement_simulation with the cameras' tracks already concatenated (pack_sim_frame)."""
        ncam = len(camids)
        cam = (C.c_int * ncam)(*camids)
        cnt = (C.c_int * ncam)(*[int(c) for c in counts])
        rc = self._call("feed_simulation", self._h, C.c_double(t), ncam, cam, cnt,
                        ids.ctypes.data_as(C.POINTER(C.c_uint64)), uv.ctypes.data_as(C.POINTER(C.c_float)))
        if rc == N.E_STATE and allow_uninit:
            return rc
        self._check(rc, "feed_measurement_simulation")
        return rc

    def feed_measurement_camera(self, t, camids, images, masks=None, allow_uninit=False):
        """VioManager::feed_measurement_camera: images[i] is a u8 (H, W) array for camera camids[i]."""
        ncam = len(camids)
        imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
        cam = (C.c_int * ncam)(*camids)
        ptrs = (C.POINTER(C.c_uint8) * ncam)(*[im.ctypes.data_as(C.POINTER(C.c_uint8)) for im in imgs])
        strides = (C.c_int * ncam)(*[im.strides[0] for im in imgs])
        mptr = None
        if masks is not None:
            mk, mptr = _mask_ptrs(masks, ncam)
        rc = self._call("feed_camera", self._h, C.c_double(t), ncam, cam, ptrs, strides, mptr)
        if rc == N.E_STATE and allow_uninit:
            return rc
        self._check(rc, "feed_measurement_camera")
        return rc

    def feed_measurement_camera_device(self, t, camids, images, masks=None, allow_uninit=False):
        """feed_measurement_camera with images already in HBM: images[i] is a uint8 (H, W) CUDA tensor
        (row stride = tensor stride).  The producer stream is synchronized before the call."""
        import torch
        ncam = len(camids)
        for im in images:
            if not (im.is_cuda and im.dtype == torch.uint8 and im.dim() == 2 and im.stride(1) == 1):
                raise ValueError("images must be 2-D uint8 CUDA tensors with unit column stride")
        torch.cuda.current_stream(images[0].device).synchronize()
        cam = (C.c_int * ncam)(*camids)
        ptrs = (C.c_void_p * ncam)(*[im.data_ptr() for im in images])
        strides = (C.c_int * ncam)(*[im.stride(0) for im in images])
        mptr = None
        if masks is not None:
            mk, mptr = _mask_ptrs(masks, ncam)
        rc = self._call("feed_camera_device", self._h, C.c_double(t), ncam, cam, ptrs, strides, mptr)
        if rc == N.E_STATE and allow_uninit:
            return rc
        self._check(rc, "feed_measurement_camera_device")
        return rc

    def get_tracks(self, cam):
        """(ids uint64[n], uv float32[n, 2]) of the KLT tracks of camera `cam` after the last feed."""
        n = C.c_int()
        cap = 4096
        ids = np.zeros(cap, dtype=np.uint64)
        uv = np.zeros((cap, 2), dtype=np.float32)
        self._check(self._call("get_tracks", self._h, cam, ids.ctypes.data_as(C.POINTER(C.c_uint64)),
                               uv.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(n)), "get_tracks")
        return ids[:n.value].copy(), uv[:n.value].copy()

    def grid_stats(self):
        """(cells, introsort_cells): the tracker's FAST cells so far and how many had > 16 candidates (the
        cells whose selection std::sort's introsort tie order decides, Grider_GRID.h:128)."""
        c, i = C.c_uint64(), C.c_uint64()
        self._check(self._call("debug_grid_stats", self._h, C.byref(c), C.byref(i)), "debug_grid_stats")
        return int(c.value), int(i.value)

    def get_pyramid(self, cam, level):
        """(img u8 (h, w), der int16 (h, w, 2)) of the last pyramid level of camera `cam`."""
        w, h = C.c_int(), C.c_int()
        self._check(self._call("get_pyramid", self._h, cam, level, C.byref(w), C.byref(h), None, None, 0),
                    "get_pyramid")
        img = np.zeros((h.value, w.value), dtype=np.uint8)
        der = np.zeros((h.value, w.value, 2), dtype=np.int16)
        self._check(self._call("get_pyramid", self._h, cam, level, C.byref(w), C.byref(h),
                               img.ctypes.data_as(C.POINTER(C.c_uint8)), der.ctypes.data_as(C.POINTER(C.c_int16)),
                               img.size), "get_pyramid")
        return img, der

    def feed_measurement_uwb(self, t, anchor_ids, ranges):
        n = len(anchor_ids)
        ids = (C.c_uint64 * n)(*anchor_ids)
        r = (C.c_double * n)(*ranges)
        self._check(self._call("feed_uwb", self._h, C.c_double(t), n, ids, r), "feed_measurement_uwb")

    def try_to_initialize_uwb_anchors(self, anchors):
        n = len(anchors)
        arr = (N.Anchor * max(n, 1))(*anchors)
        self._check(self._call("init_anchors", self._h, n, arr), "try_to_initialize_uwb_anchors")

    # ---- updater-level boundary (include/uvio_hp.h; UpdaterMSCKF.h:68, UpdaterSLAM.h:70-87, UpdaterUWB.h:55) ----
    @staticmethod
    def pack_features(features):
        """features: [(featid, [(cam, t, u, v, un, vn), ...]), ...] in observation order -> flat C arrays"""
        ids = (C.c_uint64 * max(len(features), 1))(*[int(f[0]) for f in features])
        offs, meas = [0], []
        for _, ms in features:
            for (cam, t, u, v, un, vn) in ms:
                meas.append(N.FeatMeas(int(cam), float(t), float(u), float(v), float(un), float(vn)))
            offs.append(len(meas))
        off = (C.c_int * len(offs))(*offs)
        arr = (N.FeatMeas * max(len(meas), 1))(*meas)
        return ids, off, arr

    def set_state(self, val, fej, P):
        """Adopt a state snapshot (mean, first estimates, covariance) in this state's layout."""
        val = np.ascontiguousarray(val, dtype=np.float64)
        fej = np.ascontiguousarray(fej, dtype=np.float64)
        P = np.ascontiguousarray(P, dtype=np.float64)
        self._check(self._call("set_state", self._h, _dp(val), _dp(fej), val.size, _dp(P), P.shape[0], P.shape[0]),
                    "set_state")

    def propagate_and_clone(self, t):
        self._check(self._call("propagate_and_clone", self._h, C.c_double(t)), "propagate_and_clone")

    def _updater(self, name, features):
        ids, off, arr = self.pack_features(features)
        out = (N.FeatResult * max(len(features), 1))()
        self._check(self._call(name, self._h, len(features), ids, off, arr, out), name)
        return [{"featid": int(o.featid), "status": o.status, "used": o.status == 0, "to_delete": bool(o.to_delete),
                 "p_FinG": np.array(o.p_FinG[:]), "chi2": o.chi2} for o in out[:len(features)]]

    def msckf_update(self, features):
        """UpdaterMSCKF::update on the current state; one result dict per feature"""
        return self._updater("msckf_update", features)

    def slam_update(self, features):
        """UpdaterSLAM::update (the features must be SLAM landmarks of the state)"""
        return self._updater("slam_update", features)

    def slam_delayed_init(self, features):
        """UpdaterSLAM::delayed_init: accepted features become SLAM landmarks"""
        return self._updater("slam_delayed_init", features)

    def slam_change_anchors(self):
        self._check(self._call("slam_change_anchors", self._h), "slam_change_anchors")

    def marginalize_slam(self):
        self._check(self._call("marginalize_slam", self._h), "marginalize_slam")

    def marginalize_old_clone(self):
        self._check(self._call("marginalize_old_clone", self._h), "marginalize_old_clone")

    def uwb_update_single(self, t, anchor_id, rng):
        """UpdaterUWB::update_single; True when the range passed the chi2 test and updated the state"""
        a = C.c_int(0)
        self._check(self._call("uwb_update_single", self._h, C.c_double(t), C.c_uint64(int(anchor_id)),
                               C.c_double(rng), C.byref(a)), "uwb_update_single")
        return bool(a.value)

    # ---- a measurement of the caller's own: propagate -> read the state -> build H -> update ----
    def propagate(self, t):
        """UVioPropagator::propagate: the state to time t (IMU clock) without a clone."""
        self._check(self._call("propagate", self._h, C.c_double(t)), "propagate")

    def measurement_update(self, blocks, H, res, R, chi2_thr=float("inf")):
        """StateHelper::EKFUpdate(state, H_order, H, res, R) behind a chi2 gate: blocks = [(covariance id, size), ...]
        (get_state_vector's meta) name H's column blocks; H is (r, sum sizes) with respect to the error state, R (r, r)
        with only its upper triangle read.  Returns {"applied", "chi2", "dx"}; dx is zeros when gated."""
        ids = np.ascontiguousarray([b[0] for b in blocks], dtype=np.int32)
        sizes = np.ascontiguousarray([b[1] for b in blocks], dtype=np.int32)
        n = int(sizes.sum()) if len(blocks) else 0
        res = np.ascontiguousarray(res, dtype=np.float64).reshape(-1)
        r = res.shape[0]
        H = np.ascontiguousarray(np.asarray(H, dtype=np.float64).reshape(r, n))
        R = np.ascontiguousarray(np.asarray(R, dtype=np.float64).reshape(r, r))
        dx = np.zeros(self.cov_dim())
        chi2, applied = C.c_double(0.0), C.c_int(0)
        ip = C.POINTER(C.c_int)
        self._check(self._call("measurement_update", self._h, len(blocks), ids.ctypes.data_as(ip),
                               sizes.ctypes.data_as(ip), _dp(H), max(n, 1), r, _dp(res), _dp(R), max(r, 1),
                               C.c_double(chi2_thr), C.byref(chi2), C.byref(applied), _dp(dx)), "measurement_update")
        return {"applied": bool(applied.value), "chi2": chi2.value, "dx": dx}

    def position_fix(self, p_meas, p_SinI, R, chi2_mult=1.0):
        """A position sensor S rigidly mounted at p_SinI (IMU frame) that measures its own position in the global
        frame: h(x) = p_IinG + R_GtoI^T p_SinI, linearized at the current values (position_fix_jacobian), gated at
        chi2_mult * chi2_95(3)."""
        x = self.get_imu_state()[1]
        pred, H = position_fix_jacobian(x[0:4], x[4:7], p_SinI)
        imu = [m for m in self.get_state_vector()[1] if m[0] == 0][0]  # kind 0: the IMU; its pose is columns 0 .. 5
        return self.measurement_update([(int(imu[1]), 6)], H, np.asarray(p_meas, dtype=np.float64) - pred, R,
                                       chi2_mult * chi2_95(3))

    # ---- state variables of the caller's own (uvio_hp_aux_*): a lever arm, a bias, a frame offset, a scale ----
    @staticmethod
    def _walk(walk_sigma, dim):
        if walk_sigma is None:
            return None, None
        w = np.ascontiguousarray(np.broadcast_to(np.asarray(walk_sigma, dtype=np.float64), (dim,)))
        return w, _dp(w)

    def add_state(self, val, prior_cov, walk_sigma=None):
        """A new additive state variable (1 .. 8 scalars) with value val and prior covariance prior_cov (upper
        triangle read), uncorrelated with the rest; walk_sigma: random-walk density per component in unit / sqrt(s)
        (None: a constant).  Needs options.max_aux_dim.  Returns the handle."""
        val = np.ascontiguousarray(val, dtype=np.float64).reshape(-1)
        d = val.size
        pr = np.ascontiguousarray(np.asarray(prior_cov, dtype=np.float64).reshape(d, d))
        w, wp = self._walk(walk_sigma, d)
        h = C.c_int(0)
        self._check(self._call("aux_add", self._h, d, _dp(val), _dp(pr), d, wp, C.byref(h)), "aux_add")
        return h.value

    def add_state_from_measurement(self, val0, blocks, H_x, H_aux, res, R, walk_sigma=None):
        """StateHelper::initialize_invertible for a caller's variable: dim rows res = H_x dx + H_aux dx_aux + noise(R),
        H_x over blocks = [(covariance id, size), ...], H_aux (dim, dim) invertible.  The value becomes
        val0 + H_aux^-1 res, correlated with the state through H_x.  Returns the handle."""
        val0 = np.ascontiguousarray(val0, dtype=np.float64).reshape(-1)
        d = val0.size
        ids = np.ascontiguousarray([b[0] for b in blocks], dtype=np.int32)
        sizes = np.ascontiguousarray([b[1] for b in blocks], dtype=np.int32)
        n = int(sizes.sum()) if len(blocks) else 0
        H_x = np.ascontiguousarray(np.asarray(H_x, dtype=np.float64).reshape(d, n))
        H_aux = np.ascontiguousarray(np.asarray(H_aux, dtype=np.float64).reshape(d, d))
        res = np.ascontiguousarray(res, dtype=np.float64).reshape(d)
        R = np.ascontiguousarray(np.asarray(R, dtype=np.float64).reshape(d, d))
        w, wp = self._walk(walk_sigma, d)
        h = C.c_int(0)
        ip = C.POINTER(C.c_int)
        self._check(self._call("aux_add_from_measurement", self._h, d, _dp(val0), len(blocks), ids.ctypes.data_as(ip),
                               sizes.ctypes.data_as(ip), _dp(H_x), max(n, 1), _dp(H_aux), d, _dp(res), _dp(R), d, wp,
                               C.byref(h)), "aux_add_from_measurement")
        return h.value

    def add_quat_state(self, q, prior_cov, walk_sigma=None):
        """A new JPL unit quaternion [x y z w] of the caller's own (a mounting rotation): 3 error dimensions, updated
        as q <- dq(dtheta) (x) q.  prior_cov (3, 3) over dtheta (upper triangle read); walk_sigma in rad / sqrt(s)
        (None: a constant).  q is normalized on entry.  Returns the handle; aux_state gives 4 values for it."""
        q = np.ascontiguousarray(q, dtype=np.float64).reshape(4)
        pr = np.ascontiguousarray(np.asarray(prior_cov, dtype=np.float64).reshape(3, 3))
        w, wp = self._walk(walk_sigma, 3)
        h = C.c_int(0)
        self._check(self._call("aux_add_quat", self._h, _dp(q), _dp(pr), 3, wp, C.byref(h)), "aux_add_quat")
        return h.value

    def aux_state(self, handle):
        """(covariance offset, value) of an aux variable now.  The offset moves when clones or landmarks in front
        of the variable are marginalized: ask before building an H.  A quaternion variable (add_quat_state) has 3
        error columns at the offset and a value of 4."""
        vid, dim = C.c_int(), C.c_int()
        val = np.full(N.AUX_MAX_DIM, np.nan)
        self._check(self._call("aux_get", self._h, int(handle), C.byref(vid), C.byref(dim), _dp(val)), "aux_get")
        # a quaternion variable reports dim = 3 and writes 4 doubles (values are always finite)
        k = 4 if dim.value == 3 and np.isfinite(val[3]) else dim.value
        return vid.value, val[:k].copy()

    def remove_state(self, handle):
        """Marginalize an aux variable; the handle is dead afterwards."""
        self._check(self._call("aux_remove", self._h, int(handle)), "aux_remove")

    def aux_count(self):
        """(number of live aux variables, sum of their dimensions)"""
        n, d = C.c_int(), C.c_int()
        self._check(self._call("aux_count", self._h, C.byref(n), C.byref(d)), "aux_count")
        return n.value, d.value

    def position_fix_lever_arm(self, p_meas, handle, R, chi2_mult=1.0):
        """position_fix with the antenna's lever arm p_AinI an aux variable (add_state): z = p_IinG + R_ItoG p_AinI,
        H over [IMU pose (6) | p_AinI (3)] (position_fix_lever_arm_jacobian), the aux offset read now."""
        x = self.get_imu_state()[1]
        aid, arm = self.aux_state(handle)
        pred, H = position_fix_lever_arm_jacobian(x[0:4], x[4:7], arm)
        imu = [m for m in self.get_state_vector()[1] if m[0] == 0][0]
        return self.measurement_update([(int(imu[1]), 6), (aid, 3)], H, np.asarray(p_meas, dtype=np.float64) - pred, R,
                                       chi2_mult * chi2_95(3))

    # ---- buffered position fixes (uvio_hp_feed_position): replayed in time order inside the next frame ----
    def feed_measurement_position(self, t, z, R, Cm=None, p_SinI=None, aux_handle=0, chi2_mult=1.0):
        """Queue the fix z = Cm (p_IinG + R_GtoI^T s) + noise(R) at time t: Cm (r, 3), r = 1 .. 3 (None: the identity),
        R (r, r) with its upper triangle read, s the constant lever arm p_SinI (None: zero) or, with aux_handle > 0, a
        3-dimensional variable of add_state.  Gated at chi2_mult * chi2_95(r) (inf: no gate).  The next camera or
        simulation feed propagates to t and applies it, merged in time order with the UWB messages.  Returns True when
        the fix was queued, False when the filter is not initialized or t is not after the state time."""
        z = np.ascontiguousarray(z, dtype=np.float64).reshape(-1)
        r = z.size
        if Cm is None and r != 3:
            raise ValueError("feed_measurement_position: a fix of %d rows needs its Cm" % r)
        Cm = np.ascontiguousarray(np.eye(3) if Cm is None else np.asarray(Cm, dtype=np.float64).reshape(r, 3))
        R = np.ascontiguousarray(np.asarray(R, dtype=np.float64).reshape(r, r))
        s = None
        if int(aux_handle) <= 0:
            s = np.ascontiguousarray(np.zeros(3) if p_SinI is None else p_SinI, dtype=np.float64).reshape(3)
        queued = C.c_int(0)
        self._check(self._call("feed_position", self._h, C.c_double(t), r, _dp(Cm), _dp(z), _dp(R), max(r, 1),
                               None if s is None else _dp(s), int(aux_handle), C.c_double(chi2_mult),
                               C.byref(queued)), "feed_measurement_position")
        return bool(queued.value)

    # ---- buffered pose fixes (uvio_hp_feed_pose) ----
    def feed_measurement_pose(self, t, z_q, R, z_p=None, q_ItoS=None, rot_handle=0, p_SinI=None, arm_handle=0,
                              chi2_mult=1.0):
        """Queue the pose fix of a sensor frame S at time t: z_q = q_GtoS (JPL [x y z w]) and, with z_p = p_SinG given,
        the position too (R (6, 6), orientation rows first; without z_p R is (3, 3)).  The mounting rotation is the
        constant q_ItoS (None: identity) or, with rot_handle > 0, a variable of add_quat_state; the lever arm the
        constant p_SinI (None: zero) or, with arm_handle > 0, a 3-dimensional variable of add_state.  Gated at
        chi2_mult * chi2_95(r) (inf: no gate).  Replayed inside the next camera or simulation feed in time order with
        the UWB messages and the position fixes.  Returns True when queued."""
        full = z_p is not None
        r = 6 if full else 3
        z_q = np.ascontiguousarray(z_q, dtype=np.float64).reshape(4)
        R = np.ascontiguousarray(np.asarray(R, dtype=np.float64).reshape(r, r))
        zp = np.ascontiguousarray(z_p, dtype=np.float64).reshape(3) if full else None
        qs = None
        if int(rot_handle) <= 0:
            qs = np.ascontiguousarray([0.0, 0.0, 0.0, 1.0] if q_ItoS is None else q_ItoS, dtype=np.float64).reshape(4)
        s = None
        if int(arm_handle) <= 0:
            s = np.ascontiguousarray(np.zeros(3) if p_SinI is None else p_SinI, dtype=np.float64).reshape(3)
        queued = C.c_int(0)
        self._check(self._call("feed_pose", self._h, C.c_double(t), N.POSE_FULL if full else N.POSE_ORIENTATION,
                               _dp(z_q), None if zp is None else _dp(zp), _dp(R), r, None if qs is None else _dp(qs),
                               int(rot_handle), None if s is None else _dp(s), int(arm_handle), C.c_double(chi2_mult),
                               C.byref(queued)), "feed_measurement_pose")
        return bool(queued.value)

    def pose_results(self):
        """The pose fixes the last camera or simulation feed consumed, in processing order: a list of
        {"t", "chi2", "status"}; status 0 applied, 1 gated, 2 dropped, 3 refused."""
        n = C.c_int(0)
        rc = self._call("get_pose_results", self._h, None, None, None, 0, C.byref(n))
        if rc != N.E_CAPACITY:
            self._check(rc, "get_pose_results")
        k = n.value
        t, chi2, st = np.zeros(max(k, 1)), np.zeros(max(k, 1)), np.zeros(max(k, 1), dtype=np.int32)
        self._check(self._call("get_pose_results", self._h, _dp(t), _dp(chi2), st.ctypes.data_as(C.POINTER(C.c_int)),
                               k, C.byref(n)), "get_pose_results")
        return [{"t": float(t[i]), "chi2": float(chi2[i]), "status": int(st[i])} for i in range(k)]

    def position_results(self):
        """The fixes the last camera or simulation feed consumed, in processing order: a list of
        {"t", "chi2", "status"}; status 0 applied, 1 gated, 2 dropped, 3 refused."""
        n = C.c_int(0)
        rc = self._call("get_position_results", self._h, None, None, None, 0, C.byref(n))
        if rc != N.E_CAPACITY:
            self._check(rc, "get_position_results")
        k = n.value
        t, chi2, st = np.zeros(max(k, 1)), np.zeros(max(k, 1)), np.zeros(max(k, 1), dtype=np.int32)
        self._check(self._call("get_position_results", self._h, _dp(t), _dp(chi2), st.ctypes.data_as(C.POINTER(C.c_int)),
                               k, C.byref(n)), "get_position_results")
        return [{"t": float(t[i]), "chi2": float(chi2[i]), "status": int(st[i])} for i in range(k)]

    # ---- getters ----
    def initialized(self):
        """VioManager::initialized (VioManager.h:99): initialize_with_gt ran or an initializer succeeded."""
        out = C.c_int()
        self._check(self._call("initialized", self._h, C.byref(out)), "initialized")
        return bool(out.value)

    def get_imu_state(self):
        t = C.c_double()
        out = np.zeros(16)
        self._check(self._call("get_imu_state", self._h, C.byref(t), _dp(out)), "get_imu_state")
        return t.value, out

    def cov_dim(self):
        n = C.c_int()
        self._check(self._call("get_cov_dim", self._h, C.byref(n)), "get_cov_dim")
        return n.value

    def get_cov(self):
        n = self.cov_dim()
        P = np.zeros((n, n))
        self._check(self._call("get_cov", self._h, _dp(P), n), "get_cov")
        return P

    def get_state_vector(self):
        cap = 4096
        out = np.zeros(cap)
        meta = np.zeros(3 * 1024, dtype=np.int32)
        ln, nv = C.c_int(), C.c_int()
        self._check(self._call("get_state_vector", self._h, _dp(out), cap, C.byref(ln),
                               meta.ctypes.data_as(C.POINTER(C.c_int)), meta.size, C.byref(nv)), "get_state_vector")
        return out[:ln.value].copy(), meta[:3 * nv.value].reshape(-1, 3).copy()

    def get_fej_vector(self):
        out = np.zeros(4096)
        ln = C.c_int()
        self._check(self._call("get_fej_vector", self._h, _dp(out), out.size, C.byref(ln)), "get_fej_vector")
        return out[:ln.value].copy()

    def get_timing(self):
        return self.get_timing_raw().as_dict()

    def get_timing_raw(self):
        """the timing struct itself (uvio_hp_timing_t); .as_dict() gives get_timing()'s dict"""
        t = N.Timing()
        self._check(self._call("get_timing", self._h, C.byref(t)), "get_timing")
        return t

    def set_kernel_timing(self, period=1):
        """Live per-class device timing of the roofline kernels (HIP events, include/uvio_hp.h): the launches
        of every `period`-th frame are timed (0 = off)."""
        self._check(self._call("set_kernel_timing", self._h, int(period)), "set_kernel_timing")

    def kernel_stats(self, flush=True):
        """{class name: {kernels, bound, launches, seconds, flops, bytes}} cumulative since switched on."""
        cap = 16
        arr = (N.KStat * cap)()
        n = C.c_int()
        self._check(self._call("get_kernel_stats", self._h, 1 if flush else 0, arr, cap, C.byref(n)),
                    "get_kernel_stats")
        return {d["name"]: d for d in (arr[i].as_dict() for i in range(min(n.value, cap)))}

    def debug_last_msckf(self):
        cap = 8192
        ids = np.zeros(cap, dtype=np.uint64)
        pG = np.zeros((cap, 3))
        st = np.zeros(cap, dtype=np.int32)
        c2 = np.zeros(cap)
        n = C.c_int()
        self._check(self._call("debug_last_msckf", self._h, ids.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(pG),
                               st.ctypes.data_as(C.POINTER(C.c_int)), _dp(c2), cap, C.byref(n)), "debug_last_msckf")
        k = n.value
        return ids[:k].copy(), pG[:k].copy(), st[:k].copy(), c2[:k].copy()

    def debug_last_msckf_dx(self):
        """dx of the last UpdaterMSCKF::update, indexed by covariance id (zeros when nothing was accepted)"""
        dx = np.zeros(4096)
        n = C.c_int()
        self._check(self._call("debug_last_msckf_dx", self._h, _dp(dx), dx.size, C.byref(n)), "debug_last_msckf_dx")
        return dx[:n.value].copy()

    def debug_frame_feats(self):
        """Per-feature results of every updater call of the last frame: (kind, ids, p_FinG, status, chi2);
        kind 0 MSCKF update, 1 SLAM update, 2 delayed initialization."""
        cap = 16384
        kind = np.zeros(cap, dtype=np.int32)
        ids = np.zeros(cap, dtype=np.uint64)
        pG = np.zeros((cap, 3))
        st = np.zeros(cap, dtype=np.int32)
        c2 = np.zeros(cap)
        n = C.c_int()
        self._check(self._call("debug_frame_feats", self._h, kind.ctypes.data_as(C.POINTER(C.c_int)),
                               ids.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(pG), st.ctypes.data_as(C.POINTER(C.c_int)),
                               _dp(c2), cap, C.byref(n)), "debug_frame_feats")
        k = min(n.value, cap)
        return kind[:k].copy(), ids[:k].copy(), pG[:k].copy(), st[:k].copy(), c2[:k].copy()

    def get_active_tracks(self):
        """VioManager::get_active_tracks: (time, {featid: p_FinG}, {featid: (u, v, depth)})."""
        cap = 16384
        t = C.c_double()
        ids = np.zeros(cap, dtype=np.uint64)
        pos = np.zeros((cap, 3))
        uvd = np.zeros((cap, 3))
        ok = np.zeros(cap, dtype=np.int32)
        n = C.c_int()
        self._check(self._call("get_active_tracks", self._h, C.byref(t), ids.ctypes.data_as(C.POINTER(C.c_uint64)),
                               _dp(pos), _dp(uvd), ok.ctypes.data_as(C.POINTER(C.c_int)), cap, C.byref(n)),
                    "get_active_tracks")
        k = n.value
        P = {int(ids[i]): pos[i].copy() for i in range(k)}
        D = {int(ids[i]): uvd[i].copy() for i in range(k) if ok[i]}
        return t.value, P, D

    def get_features_slam(self):
        """VioManager::get_features_SLAM (VioManagerHelper.cpp:417): {featid: p_FinG} of every SLAM landmark, an
        anchored representation transformed through its anchor clone and camera."""
        n = C.c_int()
        rc = self._call("get_features_slam", self._h, None, None, 0, C.byref(n))  # the count first
        if rc != N.E_CAPACITY:
            self._check(rc, "get_features_slam")
        cap = max(n.value, 1)
        ids = np.zeros(cap, dtype=np.uint64)
        pos = np.zeros((cap, 3))
        self._check(self._call("get_features_slam", self._h, ids.ctypes.data_as(C.POINTER(C.c_uint64)), _dp(pos), cap,
                               C.byref(n)), "get_features_slam")
        return {int(ids[i]): pos[i].copy() for i in range(n.value)}

    def get_clone_times(self):
        out = np.zeros(256)
        n = C.c_int()
        self._check(self._call("get_clone_times", self._h, _dp(out), 256, C.byref(n)), "get_clone_times")
        return out[:n.value].copy()

    # ---- what the ROS node reads after every message (ROS1Visualizer.cpp:245-327, 618, 687, 805) ----
    def get_marginal_cov(self, blocks, ld=None):
        """StateHelper::get_marginal_covariance: blocks = [(covariance id, size), ...] (get_state_vector's meta
        columns 1 and 2), in any order, repeats allowed -> the (m, m) marginal, gathered on the device.  ld: the
        leading dimension handed to the library (default m)."""
        ids = np.ascontiguousarray([b[0] for b in blocks], dtype=np.int32)
        sizes = np.ascontiguousarray([b[1] for b in blocks], dtype=np.int32)
        m = int(sizes.sum()) if len(blocks) else 0
        ld = m if ld is None else int(ld)
        out = np.zeros((m, max(ld, 1)))
        ip = C.POINTER(C.c_int)
        self._check(self._call("get_marginal_cov", self._h, len(blocks), ids.ctypes.data_as(ip), sizes.ctypes.data_as(ip),
                               _dp(out), ld), "get_marginal_cov")
        return out[:, :m].copy()

    def get_good_features_msckf(self):
        """VioManager::get_good_features_MSCKF: (n, 3) p_FinG of the features the last MSCKF updates kept."""
        n = C.c_int()
        cap = 8192
        out = np.zeros((cap, 3))
        self._check(self._call("get_good_features_msckf", self._h, _dp(out), cap, C.byref(n)), "get_good_features_msckf")
        return out[:n.value].copy()

    def enable_odometry(self, on=True):
        """Switch the IMU-rate odometry cache on / off (off by default)."""
        self._check(self._call("odometry_enable", self._h, 1 if on else 0), "odometry_enable")

    def fast_state_propagate(self, t):
        """Propagator::fast_state_propagate: (state_plus (13,), cov (12, 12)) at IMU time t, or None where the
        reference returns false.  May be called from another thread beside the feeds."""
        sp = np.zeros(13)
        cov = np.zeros((12, 12))
        ok = C.c_int(0)
        rc = self._call("fast_state_propagate", self._h, C.c_double(t), _dp(sp), _dp(cov), C.byref(ok))
        if rc != 0:  # (the call leaves the handle's error message alone)
            raise RuntimeError("fast_state_propagate failed: %s" % N.ERRNAMES.get(rc, rc))
        return (sp, cov) if ok.value else None

    # ---- image products (ROS1Visualizer's trackhist and loop-closure depth images) ----
    OVERLAYS = {0: "", 1: "init", 2: "zvupt"}

    def get_track_image(self, device=False):
        """VioManager::get_historical_viz_image: (canvas uint8 (h, ncam * w, 3), overlay code) -- the canvas of
        TrackBase::display_history without the text (overlay 0: "CAM:k", 1: "init", 2: "zvupt"); the canvas is
        (0, 0, 3) before the first camera feed.  device=True: rendered into a torch uint8 tensor on the handle's
        device and returned as such."""
        w, h, ov = C.c_int(), C.c_int(), C.c_int()
        self._check(self._call("get_track_image", self._h, None, 0, C.byref(w), C.byref(h), C.byref(ov)),
                    "get_track_image")
        shape = (h.value, w.value, 3)
        nbytes = 3 * w.value * h.value
        if nbytes == 0:
            return np.zeros(shape, dtype=np.uint8), ov.value
        if device:
            import torch
            dev = torch.device("cuda", self._device)  # the handle's device, whatever torch's current one is
            out = torch.empty(shape, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            self._check(self._call("get_track_image_device", self._h, C.c_void_p(out.data_ptr()), nbytes, C.byref(w),
                                   C.byref(h), C.byref(ov)), "get_track_image_device")
            return out, ov.value
        out = np.zeros(shape, dtype=np.uint8)
        self._check(self._call("get_track_image", self._h, out.ctypes.data_as(C.POINTER(C.c_uint8)), nbytes,
                               C.byref(w), C.byref(h), C.byref(ov)), "get_track_image")
        return out, ov.value

    def get_track_history(self, cam, featid):
        """(uv float32 (n, 2) oldest first, n_cams, to_delete): Feature::uvs[cam], Feature::uvs.size() and
        Feature::to_delete of one feature of the handle's database; n = 0 when the feature is unknown."""
        n, nc, td = C.c_int(), C.c_int(), C.c_int()
        cap = 256
        while True:
            uv = np.zeros((cap, 2), dtype=np.float32)
            rc = self._call("get_track_history", self._h, cam, int(featid), uv.ctypes.data_as(C.POINTER(C.c_float)),
                            cap, C.byref(n), C.byref(nc), C.byref(td))
            if rc == N.E_CAPACITY and n.value > cap:
                cap = n.value
                continue
            self._check(rc, "get_track_history")
            return uv[:n.value].copy(), nc.value, td.value

    def get_loop_depth(self):
        """The two images of ROS1Visualizer::publish_loopclosure_information for camera 0: (time, depth uint16
        (h, w), viz uint8 (h, w, 3)); the images are empty when there is no camera-0 image or no active track
        time yet."""
        w, h, t = C.c_int(), C.c_int(), C.c_double()
        self._check(self._call("get_loop_depth", self._h, None, None, 0, C.byref(w), C.byref(h), C.byref(t)),
                    "get_loop_depth")
        depth = np.zeros((h.value, w.value), dtype=np.uint16)
        viz = np.zeros((h.value, w.value, 3), dtype=np.uint8)
        if depth.size:
            self._check(self._call("get_loop_depth", self._h, depth.ctypes.data_as(C.POINTER(C.c_uint16)),
                                   viz.ctypes.data_as(C.POINTER(C.c_uint8)), depth.size, C.byref(w), C.byref(h),
                                   C.byref(t)), "get_loop_depth")
        return t.value, depth, viz

    def track_image_times(self, on=True):
        """Device milliseconds (uploads, base, primitives, compose, copy out) of the last timed get_track_image,
        and switch the event timing on / off for the following calls."""
        ms = np.zeros(5)
        self._check(self._call("debug_track_image_times", self._h, 1 if on else 0, _dp(ms)), "debug_track_image_times")
        return ms


def _strided_u8(img, what):
    img = np.asarray(img)
    if img.ndim != 2 or img.dtype != np.uint8:
        raise ValueError("%s: a 2-D uint8 image" % what)
    if img.strides[1] != 1 or img.strides[0] < img.shape[1]:
        img = np.ascontiguousarray(img)
    return img


def draw_tracks(images, tracks, masks=None, stage_ms=False):
    """uvio_hp_debug_draw_tracks: the renderer of get_track_image on caller-given inputs.  images: per camera a
    2-D uint8 array (a strided view keeps its row stride); masks: None or per camera None / a uint8 array of the
    image's shape; tracks: per camera a list, in draw order, of dicts {id, u, v, highlighted, n_cams, to_delete,
    hist} with hist an (n, 2) array of the feature's (u, v) in this camera, oldest first.  Returns the canvas
    uint8 (max_h, ncam * max_w, 3) (with stage_ms, also the five device stage times in milliseconds)."""
    lib = N.load()
    ncam = len(images)
    imgs = [_strided_u8(im, "draw_tracks") for im in images]
    mks = [None] * ncam
    if masks is not None:
        for k, m in enumerate(masks):
            if m is None:
                continue
            # (the library reads a mask at its image's stride)
            buf = np.zeros((imgs[k].shape[0], imgs[k].strides[0]), dtype=np.uint8)
            buf[:, :imgs[k].shape[1]] = np.asarray(m, dtype=np.uint8)
            mks[k] = buf
    bp = C.POINTER(C.c_uint8)
    ip = C.POINTER(C.c_int)
    img_p = (bp * ncam)(*[im.ctypes.data_as(bp) for im in imgs])
    mask_p = (bp * ncam)(*[bp() if m is None else m.ctypes.data_as(bp) for m in mks])
    ws = np.array([im.shape[1] for im in imgs], dtype=np.int32)
    hs = np.array([im.shape[0] for im in imgs], dtype=np.int32)
    st = np.array([im.strides[0] for im in imgs], dtype=np.int32)
    counts = np.array([len(t) for t in tracks], dtype=np.int32)
    flat = [t for cam in tracks for t in cam]
    arr = (N.VizTrack * max(len(flat), 1))()
    uv = []
    off = 0
    for i, t in enumerate(flat):
        hist = np.asarray(t["hist"], dtype=np.float32).reshape(-1, 2)
        arr[i] = N.VizTrack(int(t["id"]), float(t["u"]), float(t["v"]), int(t["highlighted"]), int(t["n_cams"]),
                            int(t["to_delete"]), off, len(hist))
        uv.append(hist)
        off += len(hist)
    uv = np.ascontiguousarray(np.concatenate(uv) if uv else np.zeros((0, 2)), dtype=np.float32)
    if uv.size == 0:
        uv = np.zeros((1, 2), dtype=np.float32)
    w, h = C.c_int(), C.c_int()
    args = [ncam, img_p, ws.ctypes.data_as(ip), hs.ctypes.data_as(ip), st.ctypes.data_as(ip), mask_p,
            counts.ctypes.data_as(ip), arr, uv.ctypes.data_as(C.POINTER(C.c_float)), off]
    N.check(lib.uvio_hp_debug_draw_tracks(*args, None, 0, C.byref(w), C.byref(h), None), what="uvio_hp_debug_draw_tracks")
    out = np.zeros((h.value, w.value, 3), dtype=np.uint8)
    ms = np.zeros(5)
    N.check(lib.uvio_hp_debug_draw_tracks(*args, out.ctypes.data_as(bp), out.size, C.byref(w), C.byref(h),
                                          _dp(ms) if stage_ms else None), what="uvio_hp_debug_draw_tracks")
    return (out, ms) if stage_ms else out


def loop_depth(img, ids, uvd):
    """uvio_hp_debug_loop_depth: get_loop_depth's two images on a caller-given 8-bit image and tracks (ids (n,),
    uvd (n, 3) = u, v, depth) -> (depth uint16 (h, w), viz uint8 (h, w, 3))."""
    lib = N.load()
    img = _strided_u8(img, "loop_depth")
    ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
    uvd = np.ascontiguousarray(uvd, dtype=np.float64).reshape(-1, 3)
    h, w = img.shape
    depth = np.zeros((h, w), dtype=np.uint16)
    viz = np.zeros((h, w, 3), dtype=np.uint8)
    bp = C.POINTER(C.c_uint8)
    n = len(ids)
    rc = lib.uvio_hp_debug_loop_depth(img.ctypes.data_as(bp), w, h, img.strides[0], n,
                                      ids.ctypes.data_as(C.POINTER(C.c_uint64)) if n else None,
                                      _dp(uvd) if n else None, depth.ctypes.data_as(C.POINTER(C.c_uint16)),
                                      viz.ctypes.data_as(bp))
    N.check(rc, what="uvio_hp_debug_loop_depth")
    return depth, viz


def ekf_update(P, H_index, H, res, sigma2, compressed=False):
    """StateHelper::EKFUpdate on a standalone covariance, on the device (returns P_new, dx).
    compressed=True: measurement compression + EKFUpdate as UpdaterMSCKF.cpp:274-286 does it."""
    lib = N.load()
    P = np.array(P, dtype=np.float64, order="C", copy=True)
    H = np.ascontiguousarray(H, dtype=np.float64)
    res = np.ascontiguousarray(res, dtype=np.float64)
    idx = np.ascontiguousarray(H_index, dtype=np.int32)
    Nn = P.shape[0]
    r, n = H.shape
    dx = np.zeros(Nn)
    fn = lib.uvio_hp_msckf_compressed_update if compressed else lib.uvio_hp_ekf_update
    rc = fn(_dp(P), Nn, idx.ctypes.data_as(C.POINTER(C.c_int)), n, _dp(H), r, _dp(res), float(sigma2), _dp(dx))
    N.check(rc, what="uvio_hp_ekf_update")
    return P, dx


def ekf_update_R(P, H_index, H, res, R, chi2_thr=float("inf"), ldr=None):
    """StateHelper::EKFUpdate with a dense R (upper triangle read) behind a chi2 gate, on a standalone covariance, on
    the device.  Returns (P_new, dx, chi2, applied); not applied: P unchanged, dx zeros."""
    lib = N.load()
    P = np.array(P, dtype=np.float64, order="C", copy=True)
    H = np.ascontiguousarray(H, dtype=np.float64)
    res = np.ascontiguousarray(res, dtype=np.float64)
    R = np.ascontiguousarray(R, dtype=np.float64)
    idx = np.ascontiguousarray(H_index, dtype=np.int32)
    Nn = P.shape[0]
    r, n = H.shape
    dx = np.zeros(Nn)
    chi2, applied = C.c_double(0.0), C.c_int(0)
    rc = lib.uvio_hp_ekf_update_r(_dp(P), Nn, idx.ctypes.data_as(C.POINTER(C.c_int)), n, _dp(H), r, _dp(res), _dp(R),
                                  R.shape[1] if ldr is None else int(ldr), float(chi2_thr), _dp(dx), C.byref(chi2),
                                  C.byref(applied))
    if rc != 0:
        msg = (lib.uvio_hp_last_error(None) or b"").decode() if rc == N.E_ARG else ""
        raise RuntimeError("uvio_hp_ekf_update_r failed: %s %s" % (N.ERRNAMES.get(rc, rc), msg))
    return P, dx, chi2.value, bool(applied.value)


def chi2_95(dof):
    """The 95 % chi-squared quantile the reference's updaters multiply their chi2_multipler into (dof 1 .. 999)."""
    out = C.c_double(0.0)
    N.check(N.load().uvio_hp_chi2_95(int(dof), C.byref(out)), what="uvio_hp_chi2_95")
    return out.value


def quat_2_Rot(q):
    """JPL quaternion (x, y, z, w) -> rotation matrix (ov_core quat_ops.h quat_2_Rot)."""
    q = np.asarray(q, dtype=np.float64)
    x, y, z, w = q
    S = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return (2.0 * w * w - 1.0) * np.eye(3) - 2.0 * w * S + 2.0 * np.outer(q[:3], q[:3])


def position_fix_jacobian(q_GtoI, p_IinG, p_SinI):
    """h(x) = p_IinG + R_GtoI^T p_SinI and its (3, 6) Jacobian over the IMU pose's error state [dtheta, dp] (JPL left
    error, R(dtheta (x) q) ~ (I - [dtheta]x) R): H_theta = -R_GtoI^T [p_SinI]x, H_p = I.  Returns (h, H)."""
    Rm = quat_2_Rot(q_GtoI)
    s = np.asarray(p_SinI, dtype=np.float64)
    S = np.array([[0.0, -s[2], s[1]], [s[2], 0.0, -s[0]], [-s[1], s[0], 0.0]])
    return np.asarray(p_IinG, dtype=np.float64) + Rm.T @ s, np.hstack([-Rm.T @ S, np.eye(3)])


def position_fix_lever_arm_jacobian(q_GtoI, p_IinG, p_AinI):
    """position_fix_jacobian with the lever arm a state variable: h(x) = p_IinG + R_ItoG p_AinI (R_ItoG = R_GtoI^T) and
    its (3, 9) Jacobian over [dtheta, dp, dp_AinI]: [-R_ItoG [p_AinI]x, I, R_ItoG].  Returns (h, H)."""
    h, H = position_fix_jacobian(q_GtoI, p_IinG, p_AinI)
    return h, np.hstack([H, quat_2_Rot(q_GtoI).T])


def _padded(P, rows, ld):
    """P in the top-left corner of a (rows, ld) array whose other entries are a recognizable padding"""
    P = np.asarray(P, dtype=np.float64)
    buf = np.full((rows, ld), -7.25)
    buf[:P.shape[0], :P.shape[1]] = P
    return buf


def aux_append_p(P, prior, ld=None):
    """uvio_hp_aux_append_p: k_aux_append on a standalone covariance.  P (N, N), prior (d, d') with d' >= d its
    leading dimension.  Returns the (N + d, ld) buffer as it came back (padding included)."""
    prior = np.ascontiguousarray(prior, dtype=np.float64)
    Nn, d = np.shape(P)[0], prior.shape[0]
    ld = Nn + d if ld is None else int(ld)
    buf = _padded(P, Nn + d, ld)
    N.check(N.load().uvio_hp_aux_append_p(_dp(buf), Nn, ld, d, _dp(prior), prior.shape[1]), what="uvio_hp_aux_append_p")
    return buf


def aux_init_p(P, H_index, H_x, H_auxinv, R, ld=None):
    """uvio_hp_aux_init_p: k_aux_init on a standalone covariance.  H_x (d, n) over the columns H_index, H_auxinv
    (d, d), R (d, d') with d' >= d.  Returns the (N + d, ld) buffer as it came back."""
    H_x = np.ascontiguousarray(H_x, dtype=np.float64)
    Hi = np.ascontiguousarray(H_auxinv, dtype=np.float64)
    R = np.ascontiguousarray(R, dtype=np.float64)
    idx = np.ascontiguousarray(H_index, dtype=np.int32)
    Nn, (d, n) = np.shape(P)[0], H_x.shape
    ld = Nn + d if ld is None else int(ld)
    buf = _padded(P, Nn + d, ld)
    rc = N.load().uvio_hp_aux_init_p(_dp(buf), Nn, ld, d, idx.ctypes.data_as(C.POINTER(C.c_int)), n, _dp(H_x),
                                     max(H_x.shape[1], 1), _dp(Hi), None, _dp(R), R.shape[1])
    N.check(rc, what="uvio_hp_aux_init_p")
    return buf


def aux_walk_p(P, ids, dims, sigma2, dt, ld=None):
    """uvio_hp_aux_walk_p: k_aux_walk on a standalone covariance.  Returns the (N, ld) buffer as it came back."""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    dims = np.ascontiguousarray(dims, dtype=np.int32)
    s2 = np.ascontiguousarray(sigma2, dtype=np.float64)
    Nn = np.shape(P)[0]
    ld = Nn if ld is None else int(ld)
    buf = _padded(P, Nn, ld)
    ip = C.POINTER(C.c_int)
    rc = N.load().uvio_hp_aux_walk_p(_dp(buf), Nn, ld, len(ids), ids.ctypes.data_as(ip), dims.ctypes.data_as(ip), _dp(s2),
                                     float(dt))
    N.check(rc, what="uvio_hp_aux_walk_p")
    return buf


def cov_propagate_p(P, s0, iold, Phi, Q, rows=None, clone_src=None, dt_id=-1, dnc=None, path=N.COV_PATH_AUTO, ld=None,
                    fill=-7.25):
    """uvio_hp_debug_cov_propagate_p: k_prop_T + k_prop_write (+ k_clone), or the fused k_prop_clone, on a standalone
    covariance.  P (N, N); the new block starts at s0, or is the indices rows (s0 ignored); Phi (p, q) over the columns
    iold, Q (p, p) whose upper triangle is read.  clone_src: the IMU pose's first index (None: no clone); dt_id >= 0
    with dnc (6) adds the time-offset term.  Returns (buf, path_ran): the (N or N + 6, ld) buffer as it came back,
    every entry outside P pre-filled with `fill`."""
    Phi = np.ascontiguousarray(Phi, dtype=np.float64)
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    iold = np.ascontiguousarray(iold, dtype=np.int32)
    p, q = Phi.shape
    if Q.shape != (p, p) or iold.shape != (q,):
        raise ValueError("Phi (p, q), Q (p, p), iold (q)")
    ip = C.POINTER(C.c_int)
    rp = None
    if rows is not None:
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        if rows.shape != (p,):
            raise ValueError("rows (p)")
        rp = rows.ctypes.data_as(ip)
    if dnc is not None:
        dnc = np.ascontiguousarray(dnc, dtype=np.float64).reshape(6)
    P = np.asarray(P, dtype=np.float64)
    Nn = P.shape[0]
    nr = Nn + (6 if clone_src is not None else 0)
    ld = nr if ld is None else int(ld)
    buf = np.full((nr, ld), fill, dtype=np.float64)
    buf[:Nn, :Nn] = P
    ran = C.c_int(-1)
    rc = N.load().uvio_hp_debug_cov_propagate_p(_dp(buf), Nn, ld, int(s0), p, rp, iold.ctypes.data_as(ip), q, _dp(Phi),
                                                _dp(Q), 0 if clone_src is None else 1,
                                                0 if clone_src is None else int(clone_src), int(dt_id),
                                                None if dnc is None else _dp(dnc), int(path), C.byref(ran))
    N.check(rc, what="uvio_hp_debug_cov_propagate_p")
    return buf, ran.value


def cov_gather_p(P, op, m0=0, ms=0, idx=None, ld=None, fill=-7.25):
    """uvio_hp_debug_cov_gather_p: k_marginalize (op N.COV_MARGINALIZE, m0, ms), k_marginalize_multi / k_compact (the
    kept indices idx) or k_marginal_gather (any idx) on a standalone covariance P (N, N) laid out at leading dimension
    ld.  Returns the output as it came back: (Nn, ld) pre-filled with `fill` for the first three, (m, m) for the
    gather."""
    P = np.asarray(P, dtype=np.float64)
    Nn = P.shape[0]
    ld = Nn if ld is None else int(ld)
    src = np.full((Nn, ld), fill, dtype=np.float64)
    src[:, :Nn] = P
    idx = np.zeros(0, dtype=np.int32) if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
    n = idx.size
    if op == N.COV_MARGINALIZE:
        out = np.full((max(Nn - int(ms), 0), ld), fill, dtype=np.float64)
    elif op == N.COV_MARGINAL_GATHER:
        out = np.full((n, n), fill, dtype=np.float64)
    else:
        out = np.full((n, ld), fill, dtype=np.float64)
    outp = out if out.size else np.zeros(1)  # (a valid pointer for an empty result)
    rc = N.load().uvio_hp_debug_cov_gather_p(_dp(src), Nn, ld, int(op), int(m0), int(ms),
                                             idx.ctypes.data_as(C.POINTER(C.c_int)), n, _dp(outp))
    N.check(rc, what="uvio_hp_debug_cov_gather_p")
    return out


def position_update_p(P, imu_id, q_GtoI, p_IinG, s, Cm, z, R, aux_id=-1, chi2_thr=float("inf"), ld=None):
    """uvio_hp_debug_position_update_p: k_fix_rows -> k_chain_M -> k_chain_update for one fix on a standalone covariance at
    the given pose.  The IMU pose's error columns start at imu_id, the lever arm s's at aux_id (< 0: a constant).
    Cm (r, 3), z (r), R (r, r') with r' >= r its leading dimension.  Returns (buf, dx, chi2, applied): the (N, ld)
    buffer as it came back (padding included); not applied: P unchanged, dx zeros."""
    z = np.ascontiguousarray(z, dtype=np.float64).reshape(-1)
    r = z.size
    Cm = np.ascontiguousarray(np.asarray(Cm, dtype=np.float64).reshape(r, 3))
    R = np.ascontiguousarray(R, dtype=np.float64)
    q = np.ascontiguousarray(q_GtoI, dtype=np.float64).reshape(4)
    p = np.ascontiguousarray(p_IinG, dtype=np.float64).reshape(3)
    s = np.ascontiguousarray(s, dtype=np.float64).reshape(3)
    Nn = np.shape(P)[0]
    ld = Nn if ld is None else int(ld)
    buf = _padded(P, Nn, ld)
    dx = np.zeros(Nn)
    chi2, applied = C.c_double(0.0), C.c_int(0)
    lib = N.load()
    rc = lib.uvio_hp_debug_position_update_p(_dp(buf), Nn, ld, int(imu_id), _dp(q), _dp(p), int(aux_id), _dp(s), r,
                                             _dp(Cm), _dp(z), _dp(R), R.shape[1], float(chi2_thr), _dp(dx),
                                             C.byref(chi2), C.byref(applied))
    N.check(rc, what="uvio_hp_debug_position_update_p")
    return buf, dx, chi2.value, bool(applied.value)


def pose_update_p(P, imu_id, q_GtoI, p_IinG, s, q_ItoS, z_q, R, z_p=None, arm_id=-1, rot_id=-1, chi2_thr=float("inf"),
                  ld=None):
    """uvio_hp_debug_pose_update_p: k_pose_rows -> k_chain_M -> k_chain_update for one pose fix on a standalone
    covariance.  The IMU pose's error columns start at imu_id, the lever arm s's at arm_id and the mounting rotation
    q_ItoS's at rot_id (< 0: a constant).  z_p None: orientation only, R (3, r'); else R (6, r'), r' >= r its leading
    dimension.  Returns (buf, dx, chi2, applied): the (N, ld) buffer as it came back (padding included); not applied: P
    unchanged, dx zeros."""
    full = z_p is not None
    R = np.ascontiguousarray(R, dtype=np.float64)
    q = np.ascontiguousarray(q_GtoI, dtype=np.float64).reshape(4)
    p = np.ascontiguousarray(p_IinG, dtype=np.float64).reshape(3)
    s = np.ascontiguousarray(s, dtype=np.float64).reshape(3)
    qs = np.ascontiguousarray(q_ItoS, dtype=np.float64).reshape(4)
    zq = np.ascontiguousarray(z_q, dtype=np.float64).reshape(4)
    zp = np.ascontiguousarray(z_p, dtype=np.float64).reshape(3) if full else None
    Nn = np.shape(P)[0]
    ld = Nn if ld is None else int(ld)
    buf = _padded(P, Nn, ld)
    dx = np.zeros(Nn)
    chi2, applied = C.c_double(0.0), C.c_int(0)
    lib = N.load()
    rc = lib.uvio_hp_debug_pose_update_p(_dp(buf), Nn, ld, int(imu_id), _dp(q), _dp(p), int(arm_id), _dp(s), int(rot_id),
                                         _dp(qs), N.POSE_FULL if full else N.POSE_ORIENTATION, _dp(zq),
                                         None if zp is None else _dp(zp), _dp(R), R.shape[1], float(chi2_thr), _dp(dx),
                                         C.byref(chi2), C.byref(applied))
    N.check(rc, what="uvio_hp_debug_pose_update_p")
    return buf, dx, chi2.value, bool(applied.value)


def compress(A):
    """R factor of [H | res] (measurement_compress_inplace semantics), on the device."""
    lib = N.load()
    A = np.ascontiguousarray(A, dtype=np.float64)
    m, nc = A.shape
    R = np.zeros((nc, nc))
    N.check(lib.uvio_hp_compress(_dp(A), m, nc - 1, _dp(R)), what="uvio_hp_compress")
    return R


def grid_order(cells, kmax=0, depth=-1):
    """Grider_GRID.h:128's std::sort as the device's FAST selection runs it (uvio_hp_debug_grid_order).
    cells: per cell the cv::FAST responses in raster order.  Returns (arrangements, tops): per cell the raster
    indices as libstdc++'s introsort loop leaves them and, for kmax > 0, the first min(n, kmax) raster indices
    of the sorted cell.  depth 0 forces the heap-sort fallback."""
    lib = N.load()
    off = np.zeros(len(cells) + 1, dtype=np.int32)
    for i, c in enumerate(cells):
        off[i + 1] = off[i] + len(c)
    resp = np.zeros(max(int(off[-1]), 1), dtype=np.uint8)
    for i, c in enumerate(cells):
        resp[off[i]:off[i + 1]] = np.asarray(c, dtype=np.int64)
    arr = np.zeros(max(int(off[-1]), 1), dtype=np.int32)
    top = np.full(max(len(cells) * kmax, 1), -1, dtype=np.int32)
    ip = C.POINTER(C.c_int)
    rc = lib.uvio_hp_debug_grid_order(resp.ctypes.data_as(C.POINTER(C.c_uint8)), off.ctypes.data_as(ip), len(cells),
                                      kmax, depth, arr.ctypes.data_as(ip), top.ctypes.data_as(ip))
    N.check(rc, what="uvio_hp_debug_grid_order")
    arrs = [arr[off[i]:off[i + 1]].copy() for i in range(len(cells))]
    tops = [top[i * kmax:i * kmax + min(kmax, len(c))].copy() for i, c in enumerate(cells)] if kmax > 0 else None
    return arrs, tops


def clahe(img):
    """histogram_method CLAHE (TrackKLT.cpp:56-67: cv::createCLAHE(10.0, Size(8, 8))->apply) of one 8-bit image
    as the tracker runs it (uvio_hp_debug_clahe: its tile-LUT kernel and level-0 kernel); both sides >= 9."""
    lib = N.load()
    img = np.asarray(img)
    if img.ndim != 2 or img.dtype != np.uint8:
        raise ValueError("clahe: a 2-D uint8 image")
    if img.strides[1] != 1 or img.strides[0] < img.shape[1]:
        img = np.ascontiguousarray(img)
    h, w = img.shape
    out = np.zeros((h, w), dtype=np.uint8)
    bp = C.POINTER(C.c_uint8)
    rc = lib.uvio_hp_debug_clahe(img.ctypes.data_as(bp), w, h, img.strides[0], out.ctypes.data_as(bp))
    N.check(rc, what="uvio_hp_debug_clahe")
    return out


def undistort(cam, uv, return_ambiguous=False):
    """CamBase::undistort_f (CamBase.h:89) of n pixel points on the device (uvio_hp_undistort); cam is a
    Camera of the options.  With return_ambiguous, also the per-point flags of the points the library
    recomputed with the host's libm tan (equidistant points next to a float rounding boundary)."""
    lib = N.load()
    uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
    out = np.zeros_like(uv)
    amb = np.zeros(uv.shape[0], dtype=np.uint8)
    intr = np.array(cam.intrinsics[:], dtype=np.float64)
    fp = C.POINTER(C.c_float)
    rc = lib.uvio_hp_undistort(int(cam.model), _dp(intr), uv.shape[0], uv.ctypes.data_as(fp), out.ctypes.data_as(fp),
                               amb.ctypes.data_as(C.POINTER(C.c_uint8)))
    N.check(rc, what="uvio_hp_undistort")
    return (out, amb) if return_ambiguous else out
