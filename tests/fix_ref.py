"""The buffered position fix restated in NumPy (tests/test_fix_ref.py, tests/test_gpu_position_feed.py).  NumPy only:
nothing from oracle/ or uvio_amd/.

    z = C (p_IinG + R_GtoI^T s) + noise(R),   H = C [ -R_GtoI^T [s]x | I | R_GtoI^T ]

over the error state [dtheta (JPL left), dp_IinG, ds], the last block only when the lever arm s is a state variable.
The update is meas_ref.ekf_update_R_ref over the columns [imu_id .. imu_id + 6) (+ [aux_id .. aux_id + 3)): in
numpy.longdouble the reference, in float64 the comparator whose own error scales the device's bound.
"""
from collections import namedtuple

import numpy as np

import ekf_ref as E
import meas_ref as M

LD = E.LD


def fix_model(q, p, s, C, aux, dtype=LD):
    """(pred, H) in `dtype`: pred = C (p + R^T s) (r), H (r, 6) or, with aux, (r, 9)"""
    q, p, s = (np.asarray(v, dtype=dtype) for v in (q, p, s))
    C = np.asarray(C, dtype=dtype).reshape(-1, 3)
    Rt = M.quat_2_Rot(q).T
    J = [-Rt @ M.skew(s), np.eye(3, dtype=dtype)] + ([Rt] if aux else [])
    return C @ (p + Rt @ s), C @ np.hstack(J)


def fix_h(q, p, s, C):
    """the measurement function alone, for finite differences"""
    return fix_model(q, p, s, C, False)[0]


def fix_columns(imu_id, aux_id):
    idx = list(range(imu_id, imu_id + 6)) + (list(range(aux_id, aux_id + 3)) if aux_id >= 0 else [])
    return np.array(idx, dtype=np.int32)


def fix_update_ref(P, imu_id, q, p, s, C, z, R, aux_id=-1, dtype=LD):
    """(P_plus, dx, chi2) of one fix in `dtype` arithmetic, model and update"""
    pred, H = fix_model(q, p, s, C, aux_id >= 0, dtype)
    return M.ekf_update_R_ref(P, fix_columns(imu_id, aux_id), H, np.asarray(z, dtype=dtype) - pred, R, dtype=dtype)


FixCase = namedtuple("FixCase", "P imu_id aux_id q p s C z R")


def fix_case(N, r, aux_id, seed, imu_id=0):
    """ekf_ref.graded_case's covariance (eight orders of magnitude) under a random pose, lever arm and C (r, 3);
    R is meas_ref.dense_R scaled to the mean diagonal of H P_II H^T, so neither term of S drowns the other;
    z lies one S-standard-deviation-sized draw off the prediction (chi2 of order r)."""
    rng = np.random.default_rng(seed)
    P = E.graded_case(N, 6, 1, seed, 1.0).P
    q = rng.standard_normal(4)
    q = q / np.linalg.norm(q)
    if q[3] < 0:
        q = -q
    p = 5.0 * rng.standard_normal(3)
    s = rng.uniform(-1.0, 1.0, 3)
    C = rng.standard_normal((r, 3))
    pred, H = fix_model(q, p, s, C, aux_id >= 0, np.float64)
    idx = fix_columns(imu_id, aux_id)
    HPH = H @ P[np.ix_(idx, idx)] @ H.T
    R = M.dense_R(r, rng) * (np.trace(HPH) / r)
    R = np.triu(R) + np.triu(R, 1).T
    S = HPH + R
    z = pred + np.linalg.cholesky((S + S.T) / 2) @ rng.standard_normal(r)
    return FixCase(P, imu_id, aux_id, q, p, s, C, z, R)
