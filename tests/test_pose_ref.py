"""tests/pose_ref.py pinned independently of the library (CPU, NumPy only): the pose-fix model every device test of
tests/test_gpu_pose_feed.py is measured against.

* a measurement equal to the prediction has a zero residual;
* a hand-worked case: q_ItoS a 90 degree turn about z, z_q a 10 degree turn about x past the prediction, so
  r_theta = 2 sin(5 deg) e_x whatever the body's orientation; the same for -z_q (the dq.w < 0 branch);
* every column block of H against central finite differences of the residual, the state perturbed by boxplus
  (q_GtoI, q_ItoS) or addition (p, s), step 1e-6, agreement 1e-7 relative to the largest entry of the block.  H is
  the derivative at the prediction, so the orientation rows are differenced there (z_q = q^_GtoS: the residual is odd
  in the perturbation and the central difference is exact to O(h^2)); the residual falls as the estimate moves
  towards the measurement, so the difference quotient is -H;
* the position rows equal fix_ref.fix_model with C = I.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ekf_ref as E  # noqa: E402
import fix_ref as F  # noqa: E402
import meas_ref as M  # noqa: E402
import pose_ref as Q  # noqa: E402

LD = E.LD


def _state(seed):
    rng = np.random.default_rng(seed)
    q, qS = Q._rand_quat(rng), Q._rand_quat(rng)
    return q, 3.0 * rng.standard_normal(3), rng.uniform(-1.0, 1.0, 3), qS


@pytest.mark.parametrize("dtype", [np.float64, LD])
def test_the_prediction_has_a_zero_residual(dtype):
    q, p, s, qS = _state(1)
    zq = M.quat_multiply(qS, q)
    zp = p + M.quat_2_Rot(q).T @ s
    res, H = Q.pose_model(q, p, s, qS, zq, zp, Q.FULL, True, True, dtype)
    assert res.dtype == dtype and H.dtype == dtype and H.shape == (6, 12)
    assert np.max(np.abs(res)) < 4e-16
    res3, H3 = Q.pose_model(q, p, s, qS, zq, None, Q.ORIENTATION, True, True, dtype)
    assert H3.shape == (3, 9) and np.max(np.abs(res3)) < 4e-16  # no lever-arm columns without position rows


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_hand_worked_ten_degrees_about_x(sign):
    q, p, s, _ = _state(2)
    h = np.sqrt(LD(0.5))
    qS = np.array([0, 0, h, h], dtype=LD)  # 90 degrees about z
    a = np.deg2rad(LD(5.0))
    turn = np.array([np.sin(a), 0, 0, np.cos(a)], dtype=LD)  # 10 degrees about x
    pred = M.quat_multiply(qS, np.asarray(q, dtype=LD))
    zq = sign * M.quat_multiply(turn, pred)
    if sign < 0:
        # the raw product z_q (x) inv(pred) has w = z_v . pred_v + z_w pred_w < 0: the negation branch is taken
        assert zq[:3] @ pred[:3] + zq[3] * pred[3] < 0
        assert M.quat_multiply(zq, Q.quat_inv(pred))[3] > 0
    res, H = Q.pose_model(q, p, s, qS, zq, None, Q.ORIENTATION, False, True, LD)
    assert np.max(np.abs(res - np.array([2 * np.sin(a), 0, 0], dtype=LD))) < 1e-18
    Rz = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])  # JPL: R_ItoS of a +90 degree turn about z
    assert np.max(np.abs(H[:, 0:3] - Rz)) < 1e-18 and np.all(H[:, 3:6] == 0) and np.array_equal(H[:, 6:9], np.eye(3))


def _residual(q, p, s, qS, zq, zp):
    return Q.pose_model(q, p, s, qS, zq, zp, Q.FULL, True, True, LD)[0]


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_H_against_central_differences(seed):
    q, p, s, qS = (np.asarray(v, dtype=LD) for v in _state(seed))
    rng = np.random.default_rng(100 + seed)
    zq = M.quat_multiply(qS, q)  # the orientation rows are differenced at the prediction
    zp = p + M.quat_2_Rot(q).T @ s + np.asarray(rng.standard_normal(3), dtype=LD)  # the position rows anywhere
    _, H = Q.pose_model(q, p, s, qS, zq, zp, Q.FULL, True, True, LD)
    h = LD(1e-6)
    moves = [lambda e: (M.quat_boxplus(q, e), p, s, qS), lambda e: (q, p + e, s, qS),
             lambda e: (q, p, s + e, qS), lambda e: (q, p, s, M.quat_boxplus(qS, e))]
    for b, move in enumerate(moves):
        D = np.zeros((6, 3), dtype=LD)
        for k in range(3):
            e = np.zeros(3, dtype=LD)
            e[k] = h
            D[:, k] = (_residual(*move(e), zq, zp) - _residual(*move(-e), zq, zp)) / (2 * h)
        blk = H[:, 3 * b:3 * b + 3]
        err = float(np.max(np.abs(-D - blk)) / max(np.max(np.abs(blk)), LD(1.0)))
        print("POSEFD seed %d block %d err %.2e" % (seed, b, err))
        assert err < 1e-7, (b, err)
    assert np.array_equal(H[0:3, 9:12], np.eye(3)) and np.all(H[3:6, 9:12] == 0) and np.all(H[0:3, 3:9] == 0)


@pytest.mark.parametrize("arm", [False, True])
def test_position_rows_are_the_position_fix_with_C_identity(arm):
    q, p, s, qS = _state(6)
    zq, zp = Q._rand_quat(np.random.default_rng(7)), p + np.array([0.3, -0.2, 0.1])
    for dtype in (np.float64, LD):
        res, H = Q.pose_model(q, p, s, qS, zq, zp, Q.FULL, arm, False, dtype)
        pred, Hf = F.fix_model(q, p, s, np.eye(3), arm, dtype)
        assert np.array_equal(H[3:6], Hf)
        assert np.array_equal(res[3:6], np.asarray(zp, dtype=dtype) - pred)


def test_update_columns_and_case_shape():
    k = Q.pose_case(17, Q.FULL, 6, 14, seed=11)
    assert list(Q.pose_columns(0, 6, 14, Q.FULL)) == list(range(0, 9)) + [14, 15, 16]
    assert list(Q.pose_columns(0, 6, 14, Q.ORIENTATION)) == list(range(0, 6)) + [14, 15, 16]
    Pp, dx, chi2 = Q.pose_update_ref(k.P, 0, k.q, k.p, k.s, k.qS, k.zq, k.zp, k.R, k.mode, 6, 14, dtype=np.float64)
    assert Pp.shape == (17, 17) and dx.shape == (17,) and 0.0 < chi2 < 60.0
    assert np.all(np.linalg.eigvalsh((Pp + Pp.T) / 2) > 0)
