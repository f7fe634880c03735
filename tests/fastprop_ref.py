"""Propagator::fast_state_propagate (Propagator.cpp:140-267) and Propagator::select_imu_readings
(Propagator.cpp:269-393) restated in numpy: the comparison statement of the IMU-rate odometry tests (the oracle
has no fast propagation).  JPL quaternions [x y z w] as in ov_core/src/utils/quat_ops.h; the error state of the
15 x 15 is (theta, p, v, b_g, b_a) with q_true = [dtheta / 2, 1] (x) q (left error).

tests/test_fastprop_ref.py anchors the statement on closed forms and on finite differences of its own mean step.
"""
import numpy as np


# ---- quat_ops.h ----
def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def quat_2_rot(q):  # quat_ops.h:152
    x = np.asarray(q[:3], dtype=float)
    w = float(q[3])
    return (2 * w * w - 1) * np.eye(3) - 2 * w * skew(x) + 2 * np.outer(x, x)


def rot_2_quat(R):  # quat_ops.h:88
    T = np.trace(R)
    q = np.zeros(4)
    if R[0, 0] >= T and R[0, 0] >= R[1, 1] and R[0, 0] >= R[2, 2]:
        q[0] = np.sqrt((1 + 2 * R[0, 0] - T) / 4)
        q[1] = (1 / (4 * q[0])) * (R[0, 1] + R[1, 0])
        q[2] = (1 / (4 * q[0])) * (R[0, 2] + R[2, 0])
        q[3] = (1 / (4 * q[0])) * (R[1, 2] - R[2, 1])
    elif R[1, 1] >= T and R[1, 1] >= R[0, 0] and R[1, 1] >= R[2, 2]:
        q[1] = np.sqrt((1 + 2 * R[1, 1] - T) / 4)
        q[0] = (1 / (4 * q[1])) * (R[0, 1] + R[1, 0])
        q[2] = (1 / (4 * q[1])) * (R[1, 2] + R[2, 1])
        q[3] = (1 / (4 * q[1])) * (R[2, 0] - R[0, 2])
    elif R[2, 2] >= T and R[2, 2] >= R[0, 0] and R[2, 2] >= R[1, 1]:
        q[2] = np.sqrt((1 + 2 * R[2, 2] - T) / 4)
        q[0] = (1 / (4 * q[2])) * (R[0, 2] + R[2, 0])
        q[1] = (1 / (4 * q[2])) * (R[1, 2] + R[2, 1])
        q[3] = (1 / (4 * q[2])) * (R[0, 1] - R[1, 0])
    else:
        q[3] = np.sqrt((1 + T) / 4)
        q[0] = (1 / (4 * q[3])) * (R[1, 2] - R[2, 1])
        q[1] = (1 / (4 * q[3])) * (R[2, 0] - R[0, 2])
        q[2] = (1 / (4 * q[3])) * (R[0, 1] - R[1, 0])
    if q[3] < 0:
        q = -q
    return q / np.linalg.norm(q)


def exp_so3(w):  # quat_ops.h:231
    w = np.asarray(w, dtype=float)
    th = np.linalg.norm(w)
    S = skew(w)
    if th < 1e-7:
        A, B = 1.0, 0.5
    else:
        A, B = np.sin(th) / th, (1 - np.cos(th)) / (th * th)
    if th == 0:
        return np.eye(3)
    return np.eye(3) + A * S + B * (S @ S)


def Jl_so3(w):  # quat_ops.h:515
    w = np.asarray(w, dtype=float)
    th = np.linalg.norm(w)
    if th < 1e-6:
        return np.eye(3)
    a = w / th
    return (np.sin(th) / th) * np.eye(3) + (1 - np.sin(th) / th) * np.outer(a, a) + ((1 - np.cos(th)) / th) * skew(a)


def Jr_so3(w):  # quat_ops.h:537
    return Jl_so3(-np.asarray(w, dtype=float))


# ---- State::Dm / State::Tg (State.h:92-111) ----
def Dm(model, v):
    D = np.zeros((3, 3))
    if model == 0:  # kalibr: lower triangular, column-wise
        D[0, 0] = v[0]
        D[1, 0], D[1, 1] = v[1], v[3]
        D[2, 0], D[2, 1], D[2, 2] = v[2], v[4], v[5]
    else:  # rpng: upper triangular, column-wise
        D[0, 0], D[0, 1], D[0, 2] = v[0], v[1], v[3]
        D[1, 1], D[1, 2] = v[2], v[4]
        D[2, 2] = v[5]
    return D


def Tg(v):
    return np.asarray(v, dtype=float).reshape(3, 3).T.copy()  # column-wise fill


# ---- Propagator::select_imu_readings (Propagator.cpp:269-393) with warn = false; imu = [(t, wm, am), ...] ----
def _interp(a, b, t):  # Propagator::interpolate_data (Propagator.h:154)
    lam = (t - a[0]) / (b[0] - a[0])
    return (t, (1 - lam) * a[1] + lam * b[1], (1 - lam) * a[2] + lam * b[2])


def select_imu_readings(imu, time0, time1):
    prop = []
    if not imu:  # :276
        return prop
    for i in range(len(imu) - 1):
        if imu[i + 1][0] > time0 and imu[i][0] < time0:  # :290 start of the period: split
            prop.append(_interp(imu[i], imu[i + 1], time0))
            continue
        if imu[i][0] >= time0 and imu[i + 1][0] <= time1:  # :301 middle
            prop.append(imu[i])
            continue
        if imu[i + 1][0] > time1:  # :312 end of the period
            if imu[i][0] > time1 and i == 0:
                break
            elif imu[i][0] > time1:
                prop.append(_interp(imu[i - 1], imu[i], time1))
            else:
                prop.append(imu[i])
            if prop[-1][0] != time1:  # :334
                prop.append(_interp(imu[i], imu[i + 1], time1))
            break
    if not prop:  # :345
        return prop
    if prop[-1][0] != time1:  # :358 the "stretch" of the last two samples past the newest one
        prop.append(_interp(imu[-2], imu[-1], time1))
    i = 0
    while i < len(prop) - 1:  # :371 zero-dt removal
        if abs(prop[i + 1][0] - prop[i][0]) < 1e-12:
            del prop[i]
            i -= 1
        i += 1
    return prop


class Calib:
    """the IMU intrinsics of Propagator.cpp:167-172"""

    def __init__(self, imu_model=0, dw=(1, 0, 0, 1, 0, 1), da=(1, 0, 0, 1, 0, 1), tg=(0,) * 9, q_acc=(0, 0, 0, 1),
                 q_gyro=(0, 0, 0, 1)):
        self.Dw = Dm(imu_model, dw)
        self.Da = Dm(imu_model, da)
        self.Tg = Tg(tg)
        self.R_acc = quat_2_rot(np.asarray(q_acc, dtype=float))
        self.R_gyro = quat_2_rot(np.asarray(q_gyro, dtype=float))


class Noise:
    def __init__(self, sigma_w, sigma_a, sigma_wb, sigma_ab, gravity_mag):
        self.sigma_w_2, self.sigma_a_2 = sigma_w ** 2, sigma_a ** 2
        self.sigma_wb_2, self.sigma_ab_2 = sigma_wb ** 2, sigma_ab ** 2
        self.gravity = np.array([0.0, 0.0, gravity_mag])


def corrected(calib, est, wm, am):
    """(a_hat, w_hat) of one reading (Propagator.cpp:184-190)"""
    a = calib.R_acc @ calib.Da @ (am - est[13:16])
    w = calib.R_gyro @ calib.Dw @ (wm - est[10:13] - calib.Tg @ a)
    return a, w


def mean_step(est, noise, a_hat, w_hat, dt):
    """Propagator.cpp:233-236"""
    R = quat_2_rot(est[0:4])
    p, v = est[4:7], est[7:10]
    out = est.copy()
    out[0:4] = rot_2_quat(exp_so3(-w_hat * dt) @ R)
    out[4:7] = p + v * dt + 0.5 * R.T @ a_hat * dt * dt - 0.5 * noise.gravity * dt * dt
    out[7:10] = v + R.T @ a_hat * dt - noise.gravity * dt
    return out


def interval_F_G(est, a_hat, w_hat, dt):
    """Propagator.cpp:201-218"""
    R = quat_2_rot(est[0:4])
    F = np.zeros((15, 15))
    F[0:3, 0:3] = exp_so3(-w_hat * dt)
    F[0:3, 9:12] = -exp_so3(-w_hat * dt) @ Jr_so3(-w_hat * dt) * dt
    F[9:12, 9:12] = np.eye(3)
    F[6:9, 0:3] = -R.T @ skew(a_hat * dt)
    F[6:9, 6:9] = np.eye(3)
    F[6:9, 12:15] = -R.T * dt
    F[12:15, 12:15] = np.eye(3)
    F[3:6, 0:3] = -0.5 * R.T @ skew(a_hat * dt * dt)
    F[3:6, 6:9] = np.eye(3) * dt
    F[3:6, 12:15] = -0.5 * R.T * dt * dt
    F[3:6, 3:6] = np.eye(3)
    G = np.zeros((15, 12))
    G[0:3, 0:3] = -exp_so3(-w_hat * dt) @ Jr_so3(-w_hat * dt) * dt
    G[6:9, 3:6] = -R.T * dt
    G[3:6, 3:6] = -0.5 * R.T * dt * dt
    G[9:12, 6:9] = np.eye(3)
    G[12:15, 9:12] = np.eye(3)
    return F, G


class FastPropagator:
    """The cache of Propagator.h:449-453 and fast_state_propagate on it.  refresh() is what the reference does
    inside the first query after invalidate_cache() (Propagator.cpp:144-150)."""

    def __init__(self, noise):
        self.noise = noise
        self.valid = False

    def refresh(self, t, est16, cov15, t_off, calib):
        self.t = float(t)
        self.est = np.array(est16, dtype=float)
        self.cov = np.array(cov15, dtype=float).reshape(15, 15)
        self.t_off = float(t_off)
        self.calib = calib
        self.valid = True

    def query(self, imu, timestamp):
        """None where the reference returns false; else (state_plus (13,), covariance (12, 12))"""
        assert self.valid
        n, c = self.noise, self.calib
        time0 = self.t + self.t_off  # :153
        time1 = timestamp + self.t_off
        prop = select_imu_readings(imu, time0, time1)
        if len(prop) < 2:  # :160
            return None
        for i in range(len(prop) - 1):  # :176
            dt = prop[i + 1][0] - prop[i][0]
            a1, w1 = corrected(c, self.est, prop[i][1], prop[i][2])
            a2, w2 = corrected(c, self.est, prop[i + 1][1], prop[i + 1][2])
            a_hat, w_hat = 0.5 * (a1 + a2), 0.5 * (w1 + w2)
            F, G = interval_F_G(self.est, a_hat, w_hat, dt)
            Qc = np.zeros((12, 12))  # :223-230
            Qc[0:3, 0:3] = n.sigma_w_2 / dt * np.eye(3)
            Qc[3:6, 3:6] = n.sigma_a_2 / dt * np.eye(3)
            Qc[6:9, 6:9] = n.sigma_wb_2 * dt * np.eye(3)
            Qc[9:12, 9:12] = n.sigma_ab_2 * dt * np.eye(3)
            Qd = G @ Qc @ G.T
            Qd = 0.5 * (Qd + Qd.T)
            self.cov = F @ self.cov @ F.T + Qd
            self.est = mean_step(self.est, n, a_hat, w_hat, dt)
        self.t = time1  # :241
        self.t_off = 0.0
        q = self.est[0:4]
        Rq = quat_2_rot(q)
        sp = np.zeros(13)  # :244-254
        sp[0:4] = q
        sp[4:7] = self.est[4:7]
        sp[7:10] = Rq @ self.est[7:10]
        _, last_w = corrected(c, self.est, prop[-1][1], prop[-1][2])
        sp[10:13] = last_w
        Phi = np.eye(15)  # :259-265
        Phi[6:9, 6:9] = Rq
        tmp = Phi @ self.cov @ Phi.T
        cov = np.zeros((12, 12))
        cov[0:9, 0:9] = tmp[0:9, 0:9]
        dt = prop[-1][0] - prop[-2][0]
        cov[9:12, 9:12] = n.sigma_w_2 / dt * np.eye(3)
        return sp, cov
