"""Anchors of tests/fastprop_ref.py, the numpy restatement of Propagator::fast_state_propagate
(Propagator.cpp:140-267) the odometry tests compare against: closed forms for the mean, and every block of one
interval's F against central finite differences of the restated mean step.  Identity IMU intrinsics throughout,
where the reference's F is the exact linearization of its mean (no correlation with the intrinsics is tracked,
Propagator.cpp:199)."""
import numpy as np

import fastprop_ref as FR

NOISE = FR.Noise(1.7e-4, 2.0e-3, 1.9e-5, 3.0e-3, 9.81)


def _samples(t0, n, dt, wm, am):
    return [(t0 + k * dt, np.array(wm, dtype=float), np.array(am, dtype=float)) for k in range(n)]


def _fresh(est, t=10.0, t_off=0.0):
    fp = FR.FastPropagator(NOISE)
    fp.refresh(t, est, 1e-4 * np.eye(15), t_off, FR.Calib())
    return fp


def test_constant_acceleration_closed_form():
    """no rotation, constant specific force: p and v are the closed forms (the discrete step is exact for them)"""
    est = np.zeros(16)
    est[3] = 1.0
    est[4:7] = [1.0, -2.0, 0.5]
    est[7:10] = [0.3, 0.1, -0.2]
    est[13:16] = [0.02, -0.01, 0.03]  # b_a
    am = np.array([0.7, -0.4, 9.81 + 0.25])
    imu = _samples(9.99, 60, 0.005, [0, 0, 0], am)
    fp = _fresh(est)
    T = 0.2
    sp, cov = fp.query(imu, 10.0 + T)
    a = am - est[13:16] - np.array([0, 0, 9.81])
    assert np.allclose(sp[0:4], [0, 0, 0, 1], atol=1e-15)
    assert np.allclose(sp[4:7], est[4:7] + est[7:10] * T + 0.5 * a * T * T, rtol=0, atol=1e-13)
    assert np.allclose(sp[7:10], est[7:10] + a * T, rtol=0, atol=1e-13)  # R = I: local = global
    assert np.allclose(sp[10:13], 0, atol=0)
    assert np.allclose(cov, cov.T, atol=1e-18) and np.all(np.linalg.eigvalsh(cov[:9, :9]) > 0)


def test_constant_rate_about_z_closed_form():
    """a constant rate w about z from the identity: q_GtoI = [0, 0, sin(w T / 2), cos(w T / 2)] (JPL)"""
    est = np.zeros(16)
    est[3] = 1.0
    est[10:13] = [0.0, 0.0, 0.01]  # b_g
    wz = 0.8
    imu = _samples(9.99, 80, 0.005, [0, 0, wz + 0.01], [0, 0, 9.81])
    fp = _fresh(est)
    T = 0.3
    sp, _ = fp.query(imu, 10.0 + T)
    assert np.allclose(sp[0:4], [0, 0, np.sin(wz * T / 2), np.cos(wz * T / 2)], rtol=0, atol=1e-13)
    assert np.allclose(sp[10:13], [0, 0, wz], rtol=0, atol=1e-15)
    # the specific force is vertical and cancels gravity: the IMU stays where it is
    assert np.allclose(sp[4:10], 0, atol=1e-13)


def _boxplus(est, dx):
    """the 15-dimensional error state on [q p v bg ba]: left quaternion error, additive rest (IMU.h)"""
    out = est.copy()
    out[0:4] = FR.rot_2_quat(FR.exp_so3(-dx[0:3]) @ FR.quat_2_rot(est[0:4]))
    out[4:16] += dx[3:15]
    return out


def _boxminus(est_a, est_b):
    M = FR.quat_2_rot(est_a[0:4]) @ FR.quat_2_rot(est_b[0:4]).T  # exp(-dtheta) = I - skew(dtheta) + ...
    A = 0.5 * (M - M.T)
    dth = -np.array([A[2, 1], A[0, 2], A[1, 0]])
    return np.r_[dth, est_a[4:16] - est_b[4:16]]


def test_interval_F_matches_finite_differences_of_the_mean_step():
    """theta, p, v rows against every column (theta, p, v, b_g, b_a) of one interval's F: central differences of
    the restated mean step with the step (1e-6) and bound (2e-9) of tests/test_fd_goldens.py's propagation test,
    whose F is likewise the exact linearization of its mean"""
    rng = np.random.default_rng(11)
    est = np.zeros(16)
    est[0:4] = FR.rot_2_quat(FR.exp_so3(np.array([0.3, -0.5, 0.8])))
    est[4:7] = rng.standard_normal(3)
    est[7:10] = rng.standard_normal(3)
    est[10:13] = 0.01 * rng.standard_normal(3)
    est[13:16] = 0.05 * rng.standard_normal(3)
    calib = FR.Calib()
    dt = 0.005
    m = (10.0, np.array([0.3, -0.2, 0.5]), np.array([0.4, -0.3, 9.6]))
    p = (10.0 + dt, np.array([0.35, -0.1, 0.45]), np.array([0.6, -0.2, 9.9]))

    def step(e):
        a1, w1 = FR.corrected(calib, e, m[1], m[2])
        a2, w2 = FR.corrected(calib, e, p[1], p[2])
        return FR.mean_step(e, NOISE, 0.5 * (a1 + a2), 0.5 * (w1 + w2), dt)

    a1, w1 = FR.corrected(calib, est, m[1], m[2])
    a2, w2 = FR.corrected(calib, est, p[1], p[2])
    F, _ = FR.interval_F_G(est, 0.5 * (a1 + a2), 0.5 * (w1 + w2), dt)
    x1 = step(est)
    e = 1e-6
    worst = 0.0
    for j in range(15):
        dx = np.zeros(15)
        dx[j] = e
        fd = (_boxminus(step(_boxplus(est, dx)), x1) - _boxminus(step(_boxplus(est, -dx)), x1)) / (2 * e)
        worst = max(worst, np.abs(fd[0:9] - F[0:9, j]).max())
        # the bias rows are the identity
        assert np.allclose(fd[9:15], F[9:15, j], atol=2e-9)
    assert worst < 2e-9, worst
    # the blocks the statement fills are not trivially zero
    assert np.abs(F[0:3, 9:12]).max() > 1e-3 and np.abs(F[6:9, 0:3]).max() > 1e-2 and np.abs(F[3:6, 12:15]).max() > 1e-6


def test_select_imu_readings_shapes():
    """the branches of select_imu_readings the odometry query meets"""
    imu = _samples(0.0, 5, 0.1, [0, 0, 1], [1, 0, 0])
    imu = [(t, w * (1 + t), a) for t, w, a in imu]
    # both ends interpolated
    pr = FR.select_imu_readings(imu, 0.05, 0.27)
    assert [round(s[0], 12) for s in pr] == [0.05, 0.1, 0.2, 0.27]
    assert np.allclose(pr[0][1], [0, 0, 1.05]) and np.allclose(pr[-1][1], [0, 0, 1.27])
    # a query exactly on a sample ends on it, without a zero-length interval
    pr = FR.select_imu_readings(imu, 0.05, imu[2][0])
    assert [s[0] for s in pr][-1] == imu[2][0] and len(pr) == 3
    # past the newest sample: the last two samples are stretched
    pr = FR.select_imu_readings(imu, 0.05, 0.47)
    assert pr[-1][0] == 0.47 and np.allclose(pr[-1][1], [0, 0, 1.47])
    # nothing to integrate
    assert FR.select_imu_readings([], 0.0, 1.0) == []
    assert FR.select_imu_readings(imu[:1], 0.0, 1.0) == []
    assert len(FR.select_imu_readings(imu, 1.0, 1.2)) < 2
