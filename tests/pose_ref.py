"""The buffered pose fix restated in NumPy (tests/test_pose_ref.py, tests/test_gpu_pose_feed.py).  NumPy only: nothing
from oracle/ or uvio_amd/.

A sensor frame S is mounted on the body with the rotation q_ItoS and the lever arm s = p_SinI; z_q = q_GtoS and
z_p = p_SinG are reported in G.  With the JPL left error for both quaternions,

    q^_GtoS = q_ItoS (x) q_GtoI                      p^ = p_IinG + R_GtoI^T s
    r_theta = 2 vec(z_q (x) inv(q^_GtoS)), w >= 0    r_p = z_p - p^
    H_theta = [ R_ItoS | 0 | 0 | I ]                 H_p = [ -R_GtoI^T [s]x | I | R_GtoI^T | 0 ]

over the error state [dtheta, dp_IinG, ds, dphi]: the ds block only when the lever arm is a state variable (and only in
FULL mode: the orientation rows do not see it), the dphi block only when the mounting rotation is one.  Orientation rows
first.  The update is meas_ref.ekf_update_R_ref over the columns [imu_id .. + 6) (+ [arm_id .. + 3)) (+ [rot_id .. + 3)):
in numpy.longdouble the reference, in float64 the comparator whose own error scales the device's bound.
"""
from collections import namedtuple

import numpy as np

import ekf_ref as E
import meas_ref as M

LD = E.LD
ORIENTATION, FULL = 1, 2  # UVIO_HP_POSE_ORIENTATION, UVIO_HP_POSE_FULL


def quat_inv(q):
    return np.concatenate([-q[:3], q[3:4]])


def unit(q, dtype):
    q = np.asarray(q, dtype=dtype)
    return q / np.sqrt(q @ q)


def pose_model(q, p, s, q_ItoS, z_q, z_p, mode, arm, rot, dtype=LD):
    """(res, H) in `dtype`: r = 3 (ORIENTATION) or 6 (FULL) rows over 6 (+ 3 with arm in FULL mode) (+ 3 with rot)
    columns.  z_q and q_ItoS are normalized first, as the library does on entry."""
    q, p, s = (np.asarray(v, dtype=dtype) for v in (q, p, s))
    qS, zq = unit(q_ItoS, dtype), unit(z_q, dtype)
    full = mode == FULL
    arm = arm and full
    RS = M.quat_2_Rot(qS)
    dq = M.quat_multiply(zq, quat_inv(M.quat_multiply(qS, q)))  # w >= 0
    Z, I3 = np.zeros((3, 3), dtype=dtype), np.eye(3, dtype=dtype)
    res = [2 * dq[:3]]
    Ht = [RS, Z] + ([Z] if arm else []) + ([I3] if rot else [])
    rows = [np.hstack(Ht)]
    if full:
        Rt = M.quat_2_Rot(q).T
        res.append(np.asarray(z_p, dtype=dtype) - (p + Rt @ s))
        rows.append(np.hstack([-Rt @ M.skew(s), I3] + ([Rt] if arm else []) + ([Z] if rot else [])))
    return np.concatenate(res), np.vstack(rows)


def pose_columns(imu_id, arm_id, rot_id, mode):
    idx = list(range(imu_id, imu_id + 6))
    if arm_id >= 0 and mode == FULL:
        idx += list(range(arm_id, arm_id + 3))
    if rot_id >= 0:
        idx += list(range(rot_id, rot_id + 3))
    return np.array(idx, dtype=np.int32)


def pose_update_ref(P, imu_id, q, p, s, q_ItoS, z_q, z_p, R, mode, arm_id=-1, rot_id=-1, dtype=LD):
    """(P_plus, dx, chi2) of one pose fix in `dtype` arithmetic, model and update"""
    res, H = pose_model(q, p, s, q_ItoS, z_q, z_p, mode, arm_id >= 0, rot_id >= 0, dtype)
    return M.ekf_update_R_ref(P, pose_columns(imu_id, arm_id, rot_id, mode), H, res, R, dtype=dtype)


PoseCase = namedtuple("PoseCase", "P imu_id arm_id rot_id mode q p s qS zq zp R")


def _rand_quat(rng):
    q = rng.standard_normal(4)
    q = q / np.linalg.norm(q)
    return -q if q[3] < 0 else q


def pose_case(N, mode, arm_id, rot_id, seed, imu_id=0):
    """fix_ref.fix_case for a pose: ekf_ref.graded_case's covariance (eight orders of magnitude) under a random pose,
    lever arm and mounting rotation; R is meas_ref.dense_R scaled to the mean diagonal of H P_II H^T; the measurement
    lies one S-sized draw d off the prediction: z_q = dq(d[:3]) (x) q^_GtoS (boxplus), z_p = p^ + d[3:]."""
    rng = np.random.default_rng(seed)
    P = E.graded_case(N, 6, 1, seed, 1.0).P
    q, qS = _rand_quat(rng), _rand_quat(rng)
    p = 5.0 * rng.standard_normal(3)
    s = rng.uniform(-1.0, 1.0, 3)
    r = 6 if mode == FULL else 3
    q_pred = M.quat_multiply(qS, q)
    p_pred = p + M.quat_2_Rot(q).T @ s
    _, H = pose_model(q, p, s, qS, q_pred, p_pred, mode, arm_id >= 0, rot_id >= 0, np.float64)
    idx = pose_columns(imu_id, arm_id, rot_id, mode)
    HPH = H @ P[np.ix_(idx, idx)] @ H.T
    R = M.dense_R(r, rng) * (np.trace(HPH) / r)
    R = np.triu(R) + np.triu(R, 1).T
    S = HPH + R
    d = np.linalg.cholesky((S + S.T) / 2) @ rng.standard_normal(r)
    zq = M.quat_boxplus(q_pred, d[:3])
    zp = p_pred + d[3:] if mode == FULL else None
    return PoseCase(P, imu_id, arm_id, rot_id, mode, q, p, s, qS, zq, zp, R)
