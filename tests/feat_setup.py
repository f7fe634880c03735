"""What tests/test_feat_ref.py and tests/test_gpu_msckf_paths.py share around tests/feat_ref.py: the options of a
setup, a manager brought to K clones without a camera frame, the generated state it adopts, and the error metrics.

A manager gets initialize_with_gt, the IMU of a short simulated trajectory and K propagate_and_clone calls
(max_clone_size = K); the state it then holds gives the layout, the clone poses and the clone times.  The same
calls on the oracle and on the device give the same layout, so both adopt one generated snapshot with set_state.
"""
import os

import numpy as np

import feat_ref as F
from ekf_ref import LD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def options(setup, fej, rep, **more):
    import uvio_amd as U
    cfg, ov, K, _ = F.SETUPS[setup]
    kw = dict(ov, max_clone_size=K, do_fej=fej, feat_rep_msckf=rep, max_msckf_in_update=300, max_slam_features=0)
    kw.update(more)
    return U.load_options(os.path.join(ROOT, "configs", cfg, "estimator_config.yaml"), **kw)


def to_clones(mgrs, opts, setup):
    """initialize_with_gt, IMU and the setup's clones (feat_ref.clone_offsets; or a list of offsets in seconds) on
    every manager; returns the clone times"""
    from uvio_amd.sim import SimStream
    offs = F.clone_offsets(setup) if isinstance(setup, str) else list(setup)
    sim = SimStream(opts, duration=offs[-1] + 1.5, seed=21, spawn=1)
    times = [sim.t0 + v for v in offs]
    for m in mgrs:
        m.initialize_with_gt(sim.gt_state(sim.t0))
        keep = sim.imu_t <= times[-1] + 2.0 / sim.imu_rate
        m.feed_measurement_imu_batch(sim.imu_t[keep], sim.wm[keep], sim.am[keep])
        for t in times:
            m.propagate_and_clone(t)
        assert np.allclose(m.get_clone_times(), times)
    return times


def generated_state(mgr, opts, times, seed=77):
    """the manager's layout and clone poses as a feat_ref.State with generated first estimates and covariance"""
    val, meta = mgr.get_state_vector()
    return F.make_state(val, meta, times, F.cams_of(opts), opts.do_calib_camera_pose, opts.do_calib_camera_intrinsics,
                        seed)


def undistort_of(opts):
    from oracle import oracle as O
    return lambda c, uv: O.camera_undistort(opts.cams[c], uv)


def adopt(mgr, st):
    mgr.set_state(st.val, st.fej, st.P)


def x_err(xa, xb, st):
    """max_i |(xa boxminus xb)_i| / sqrt(P_ii): the state difference in prior standard deviations"""
    d = F.boxminus(xa, xb, st.meta, st.N, LD)
    return float(np.max(np.abs(d) / np.sqrt(np.diag(st.P).astype(LD))))


def x_err_floored(xa, xb, st):
    """x_err per component, less what storing the component in double precision costs: one ulp of a stored value
    (val + dx is rounded once), 16 * 2^-53 rad on a rotation (four quaternion components, a product and a
    normalization).  One global maximum would let the rounding of the largest stored value over its deviation (a
    focal length of 458 px at 1e-5) stand for every component."""
    d = np.abs(F.boxminus(xa, xb, st.meta, st.N, LD))
    floor = np.zeros(st.N, dtype=LD)
    off = 0
    xa = np.asarray(xa, dtype=np.float64)
    for kind, cid, size in st.meta:
        n = F.vlen(kind, size)
        if kind in (F.K_IMU, F.K_QUAT, F.K_POSE):
            floor[cid:cid + 3] = 16 * 2.0 ** -53
            floor[cid + 3:cid + size] = np.spacing(np.abs(xa[off + 4:off + n]))
        else:
            floor[cid:cid + size] = np.spacing(np.abs(xa[off:off + n]))
        off += n
    return float(np.max(np.maximum(d - floor, 0) / np.sqrt(np.diag(st.P).astype(LD))))


def oracle_dx(st, ev, sigma2):
    """dx of the oracle's own update (measurement compression for m > n, then StateHelper::EKFUpdate) of the
    reference's stacked rows ev, rounded to double.  The oracle's msckf_update returns no dx; this is the yardstick
    for what its update arithmetic loses on the same rows."""
    from oracle import oracle as O
    m, n = ev.H.shape
    _, dx = O.ekf_update(st.P, ev.idx.astype(np.int32), ev.H.astype(np.float64), ev.res.astype(np.float64), sigma2,
                         compressed=m > n)
    return dx


def positions(st, feats, ids, pG, status):
    """debug_last_msckf's output as evaluate() takes it: the triangulated position of every feature that has one
    (None otherwise) and the indices of the accepted ones"""
    by = {int(i): k for k, i in enumerate(ids)}
    p, acc = [], set()
    for j, f in enumerate(feats):
        k = by.get(f.fid)
        if k is None or status[k] in (1, 2):
            p.append(None)
            continue
        p.append(np.array(pG[k]))
        if status[k] == 0:
            acc.add(j)
    return p, acc
