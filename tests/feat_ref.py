"""Extended-precision (numpy.longdouble) restatement of the MSCKF feature batch, the reference of
tests/test_feat_ref.py and tests/test_gpu_msckf_paths.py, and the generator of their cases.  NumPy only: nothing from
oracle/ or uvio_amd/ (the camera undistortion, which is the project's, is handed in as a function).

Restated, for GLOBAL_3D (rep 0) and ANCHORED_MSCKF_INVERSE_DEPTH (rep 4), radtan and equidistant cameras:
  * UpdaterHelper::get_feature_jacobian_full / _representation (UpdaterHelper.cpp:32-424) at a GIVEN landmark
    position: residual at the current estimates, Jacobians at the first estimates under do_fej.  The reference's
    float casts are kept (CamBase.h:130: the normalized point goes to float, distort_f returns float; the device's
    are kernels_feat.hip:725-728), and so is its quirk that the distortion Jacobian is taken at the
    current-estimate (xn, yn) under FEJ too.  Every cast reports how far the extended value is from the nearest
    float rounding midpoint, in float ulps (Casts): a value within 1e-6 ulp of a midpoint may round either way in
    double precision.
  * the left-nullspace projection (UpdaterHelper.cpp:426-454) with Householder reflections; any orthonormal basis
    of the left nullspace gives the same chi2 and the same update
  * per feature chi2 = r^T (H P_marg H^T + sigma^2 I)^-1 r (UpdaterMSCKF.cpp:225-245)
  * the stacked rows of the accepted features through ekf_ref.ekf_update_ref, and x + dx with JPL quaternions
    (Type::update: q <- normalize([dtheta / 2, 1]) (x) q)
  * FeatureInitializer::single_triangulation (FeatureInitializer.cpp:30-112): the linear solution with its
    condition number, its depth in the anchor camera and the baseline ratio at that solution, so that a case can
    be shown to sit clear of every threshold.  The Levenberg-Marquardt refinement is not restated (it stops on
    float residuals; the oracle is its yardstick).

Every routine takes a dtype, so the same text also runs in float64: that run against the longdouble run is what
double-precision arithmetic alone costs.

The generator takes no stream: a state layout (get_state_vector's values and meta, the clone times, the cameras)
becomes a State whose first estimates sit 1e-3 off the values on the clones and the extrinsics and whose
covariance is graded as ekf_ref.graded_case grades it; landmarks are projected exactly into chosen clones and
cameras, get 1 px of noise (less on features of many rows, see _ok_views) and a float cast.  The rejected features
are built: status 1 from views of one camera pose (condition number far above fi_max_cond_number), status 2 from two
far views that agree with an infinite depth around a short baseline that agrees with a near one (the refinement runs
to a depth beyond fi_max_dist, see _depth_views), status 3 from a 50 px outlier.

CASES is the one case list of the CPU and the GPU tests.  The sizes are computed here from the device's dispatch
rules, restated below (DISPATCH RULES) with the file and the function or constant each comes from; those names are
given rather than line numbers, which move with every edit of a kernel file.  Nothing is typed in.
"""
import itertools
from collections import namedtuple

import numpy as np

from ekf_ref import HAVE_EXTENDED, LD, REASON, chol_ld, ekf_update_ref, fwd_ld  # noqa: F401

K_IMU, K_VEC, K_QUAT, K_POSE = 0, 1, 2, 3
F32 = np.float32

# ---- DISPATCH RULES (restated from the device code) ----
K_MAX_MEAS_PER_FEAT = 64        # kernels.h:20 kMaxMeasPerFeat (one lane per measurement in k_feature's geometry wave)
K_MAX_DYN_LDS = 152 * 1024      # kernels.h kMaxDynLds: the LDS budget launch_chi2_batch compares chi2_lds_bytes with
K_FEATURE_LDS = 156 * 1024      # kernels_feat.hip feature_lds_limit: what k_feature asks set_dyn_lds for
K_TILED_ROWS = 4096             # kernels_chi2.hip launch_chi2_batch: m >= 4096 -> k_gemm_HPg_tiled
K_CHUNKED_BUILD = 256           # engine_update.cpp add_features_to_batch: nf < 256 is built sequentially (and any
#                                 batch when the host pool has one thread, UVIO_HP_THREADS = 1)
K_MAX_CANON = 512               # kernels.h kMaxCanonCols (k_feature's canon2loc table)


def chi2_lds_bytes(R, n):
    """kernels_chi2.hip chi2_lds_bytes: H and T rows, S and the solve's vectors of an R-row feature"""
    return (2 * R * (n | 1) + (R + 1) * (R | 1) + 4 * (R + 1)) * 8


def chi2_instance(R):
    """kernels_chi2.hip chi2_instance: smax = (R + 1 + 63) / 64 selects k_chi2<smax>"""
    return min(max((R + 1 + 63) // 64, 1), 4)


def feature_lds_bytes(max_meas, max_nf):
    """kernels_feat.hip:311-321 feat_lds_doubles: Hl, Hf, V, loc2pid, scratch"""
    rows = 2 * max_meas
    return (rows * (max_nf + 1) + rows * 3 + rows * 3 + max_nf + 64) * 8


def rows_of(m):
    """projected rows of an m-measurement MSCKF feature (kernels.h feat_rows_out, mode 0)"""
    return 2 * m - 3


def dispatch(meas_counts, n):
    """The kernels an MSCKF batch of these feature sizes over n state columns reaches, from the rules above and
    engine_chain.cpp enqueue_update (m > n or m > 255 rows: Gram + information form, else the direct update)."""
    R = max(rows_of(m) for m in meas_counts)
    rows = sum(rows_of(m) for m in meas_counts)
    return {"rows": rows, "n": n, "gemm": "k_gemm_HPg_tiled" if rows >= K_TILED_ROWS else "k_gemm_HPg",
            "chi2": "k_chi2<%d>" % chi2_instance(R),
            "S": "LDS" if chi2_lds_bytes(R, n) <= K_MAX_DYN_LDS else "k_chi2_S2",
            "update": "information" if (rows > n or rows > 255) else "direct",
            "build": "chunked" if len(meas_counts) >= K_CHUNKED_BUILD else "sequential"}  # (chunked: with a host pool)


# ---------------------------------------------------------------------------------------------------------------
# small algebra in a given dtype
def skew(w, dt):
    z = dt(0)
    return np.array([[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]], dtype=dt)


def skew_b(w):
    """(m, 3) -> (m, 3, 3)"""
    S = np.zeros(w.shape[:-1] + (3, 3), dtype=w.dtype)
    S[..., 0, 1], S[..., 0, 2] = -w[..., 2], w[..., 1]
    S[..., 1, 0], S[..., 1, 2] = w[..., 2], -w[..., 0]
    S[..., 2, 0], S[..., 2, 1] = -w[..., 1], w[..., 0]
    return S


def quat_rot(q, dt):
    """quat_ops.h:152, JPL, q = [x y z w]"""
    q = np.asarray(q, dtype=dt)
    qv, w = q[:3], q[3]
    return (2 * w * w - 1) * np.eye(3, dtype=dt) - 2 * w * skew(qv, dt) + 2 * np.outer(qv, qv)


def quat_mul(q, p, dt):
    """quat_ops.h quat_multiply: q (x) p, w kept non-negative, normalized"""
    q, p = np.asarray(q, dtype=dt), np.asarray(p, dtype=dt)
    qv, w = q[:3], q[3]
    Q = np.zeros((4, 4), dtype=dt)
    Q[:3, :3] = w * np.eye(3, dtype=dt) - skew(qv, dt)
    Q[:3, 3] = qv
    Q[3, :3] = -qv
    Q[3, 3] = w
    r = Q @ p
    if r[3] < 0:
        r = -r
    return r / np.sqrt(r @ r)


def vlen(kind, size):
    return size + (1 if kind in (K_IMU, K_QUAT, K_POSE) else 0)


def boxplus(x, meta, dx, dt):
    """Type::update of every variable: x (state vector), dx indexed by covariance id"""
    x = np.array(x, dtype=dt)
    dx = np.asarray(dx, dtype=dt)
    off = 0
    for kind, cid, size in meta:
        n = vlen(kind, size)
        if kind in (K_IMU, K_QUAT, K_POSE):
            dq = np.array([dx[cid] / 2, dx[cid + 1] / 2, dx[cid + 2] / 2, 1], dtype=dt)
            dq = dq / np.sqrt(dq @ dq)
            x[off:off + 4] = quat_mul(dq, x[off:off + 4], dt)
            x[off + 4:off + n] += dx[cid + 3:cid + size]
        else:
            x[off:off + n] += dx[cid:cid + size]
        off += n
    return x


def boxminus(xa, xb, meta, N, dt=LD):
    """xa - xb in the error state (covariance ids), the inverse of boxplus: dtheta = 2 vec / w of qa (x) qb^-1"""
    xa, xb = np.asarray(xa, dtype=dt), np.asarray(xb, dtype=dt)
    out = np.zeros(N, dtype=dt)
    off = 0
    for kind, cid, size in meta:
        n = vlen(kind, size)
        if kind in (K_IMU, K_QUAT, K_POSE):
            qb = xb[off:off + 4] * np.array([-1, -1, -1, 1], dtype=dt)
            d = quat_mul(xa[off:off + 4], qb, dt)
            out[cid:cid + 3] = 2 * d[:3] / d[3]
            out[cid + 3:cid + size] = xa[off + 4:off + n] - xb[off + 4:off + n]
        else:
            out[cid:cid + size] = xa[off:off + n] - xb[off:off + n]
        off += n
    return out


# ---------------------------------------------------------------------------------------------------------------
# the state
Cam = namedtuple("Cam", "model width height intrinsics q_ItoC p_IinC")


def cams_of(opts):
    """the cameras of an options struct as plain tuples"""
    return [Cam(int(c.model), int(c.width), int(c.height), tuple(c.intrinsics[:]), tuple(c.q_ItoC[:]),
                tuple(c.p_IinC[:]))
            for c in (opts.cams[i] for i in range(opts.num_cameras))]


class State:
    """values, first estimates and covariance in get_state_vector's layout.  The variables come in the order of
    State.cpp:28-166: the IMU, its intrinsics, the time offset, then per camera the extrinsic pose and the
    intrinsics (each only when calibrated), then the clones in time order."""

    def __init__(self, val, fej, meta, P, clone_times, cams, calib_ext, calib_intr):
        self.val, self.fej, self.P = np.array(val, dtype=np.float64), np.array(fej, dtype=np.float64), np.array(P)
        self.meta = [tuple(int(v) for v in m) for m in meta]
        self.clone_times = [float(t) for t in clone_times]
        self.cams, self.calib_ext, self.calib_intr = cams, bool(calib_ext), bool(calib_intr)
        self.N = sum(m[2] for m in self.meta)
        off, poses, vec8 = 0, [], []
        for kind, cid, size in self.meta:
            if kind == K_POSE:
                poses.append((cid, off))
            elif kind == K_VEC and size == 8:
                vec8.append((cid, off))
            off += vlen(kind, size)
        assert off == self.val.size == self.fej.size
        K, C = len(self.clone_times), len(cams)
        assert len(poses) == K + (C if calib_ext else 0), (len(poses), K, C)
        self.ext = poses[:C] if calib_ext else None
        self.clones = poses[-K:]
        self.intr = vec8 if calib_intr else None
        assert not calib_intr or len(vec8) == C

    def clone(self, i, fej, dt):
        """(R_GtoI, p_IinG) of clone i"""
        x = self.fej if fej else self.val
        o = self.clones[i][1]
        return quat_rot(x[o:o + 4], dt), np.asarray(x[o + 4:o + 7], dtype=dt)

    def extrinsic(self, c, dt):
        """(R_ItoC, p_IinC) of camera c: its value (the reference never reads an extrinsic's first estimate)"""
        if self.ext is None:
            return quat_rot(self.cams[c].q_ItoC, dt), np.asarray(self.cams[c].p_IinC, dtype=dt)
        o = self.ext[c][1]
        return quat_rot(self.val[o:o + 4], dt), np.asarray(self.val[o + 4:o + 7], dtype=dt)

    def intrinsics(self, c, dt):
        if self.intr is None:
            return np.asarray(self.cams[c].intrinsics, dtype=dt)
        o = self.intr[c][1]
        return np.asarray(self.val[o:o + 8], dtype=dt)

    def cam_pose(self, i, c, dt):
        """(R_GtoC, p_CinG) of camera c at clone i, current values (FeatureInitializer's ClonesCam)"""
        R, p = self.clone(i, False, dt)
        Rc, pc = self.extrinsic(c, dt)
        RG = Rc @ R
        return RG, p - RG.T @ pc


# ---------------------------------------------------------------------------------------------------------------
# cameras
class Casts:
    """the float casts of one evaluation: dist = the smallest distance of a cast value to a float rounding midpoint,
    in float ulps (0.5 = exactly representable)"""

    def __init__(self):
        self.dist = 0.5

    def f32(self, x):
        x = np.asarray(x)
        f = x.astype(F32)
        a = np.abs(f)
        # the float grid on x's side of f: coarser above |f| than below it when |f| is a power of two
        below = (a - np.nextafter(a, F32(0))).astype(LD)
        ulp = np.where(np.abs(x.astype(LD)) < a.astype(LD), below, np.spacing(a).astype(LD))
        frac = np.abs(x.astype(LD) - f.astype(LD)) / ulp
        if frac.size:
            self.dist = min(self.dist, float(np.min(0.5 - frac)))
        return f


def distort(model, v, xf, yf, dt):
    """distort_f's inside (CamRadtan.h:127 / CamEqui.h:136) on float inputs: the pixel before its float cast"""
    x, y = xf.astype(dt), yf.astype(dt)
    r = np.sqrt(x * x + y * y)
    if model == 0:
        r2 = r * r
        r4 = r2 * r2
        x1 = x * (1 + v[4] * r2 + v[5] * r4) + 2 * v[6] * x * y + v[7] * (r2 + 2 * x * x)
        y1 = y * (1 + v[4] * r2 + v[5] * r4) + v[6] * (r2 + 2 * y * y) + 2 * v[7] * x * y
    else:
        th = np.arctan(r)
        thd = th + v[4] * th ** 3 + v[5] * th ** 5 + v[6] * th ** 7 + v[7] * th ** 9
        big = r > 1e-8
        cd = np.where(big, thd / np.where(big, r, 1), 1)
        x1, y1 = x * cd, y * cd
    return v[0] * x1 + v[2], v[1] * y1 + v[3]


def distort_jacobian(model, v, x, y, dt):
    """compute_distort_jacobian (CamRadtan.h:154 / CamEqui.h:166) at (x, y), arrays of m: (m, 2, 2), (m, 2, 8)"""
    m = x.shape[0]
    dzn, dze = np.zeros((m, 2, 2), dtype=dt), np.zeros((m, 2, 8), dtype=dt)
    r = np.sqrt(x * x + y * y)
    if model == 0:
        r2 = r * r
        r4 = r2 * r2
        x2, y2, xy = x * x, y * y, x * y
        dzn[:, 0, 0] = v[0] * ((1 + v[4] * r2 + v[5] * r4) + (2 * v[4] * x2 + 4 * v[5] * x2 * r2) + 2 * v[6] * y +
                               (2 * v[7] * x + 4 * v[7] * x))
        dzn[:, 0, 1] = v[0] * (2 * v[4] * xy + 4 * v[5] * xy * r2 + 2 * v[6] * x + 2 * v[7] * y)
        dzn[:, 1, 0] = v[1] * (2 * v[4] * xy + 4 * v[5] * xy * r2 + 2 * v[6] * x + 2 * v[7] * y)
        dzn[:, 1, 1] = v[1] * ((1 + v[4] * r2 + v[5] * r4) + (2 * v[4] * y2 + 4 * v[5] * y2 * r2) + 2 * v[7] * x +
                               (2 * v[6] * y + 4 * v[6] * y))
        x1 = x * (1 + v[4] * r2 + v[5] * r4) + 2 * v[6] * x * y + v[7] * (r2 + 2 * x * x)
        y1 = y * (1 + v[4] * r2 + v[5] * r4) + v[6] * (r2 + 2 * y * y) + 2 * v[7] * x * y
        dze[:, 0, 0], dze[:, 0, 2] = x1, 1
        dze[:, 0, 4], dze[:, 0, 5] = v[0] * x * r2, v[0] * x * r4
        dze[:, 0, 6], dze[:, 0, 7] = 2 * v[0] * x * y, v[0] * (r2 + 2 * x * x)
        dze[:, 1, 1], dze[:, 1, 3] = y1, 1
        dze[:, 1, 4], dze[:, 1, 5] = v[1] * y * r2, v[1] * y * r4
        dze[:, 1, 6], dze[:, 1, 7] = v[1] * (r2 + 2 * y * y), 2 * v[1] * x * y
    else:
        th = np.arctan(r)
        thd = th + v[4] * th ** 3 + v[5] * th ** 5 + v[6] * th ** 7 + v[7] * th ** 9
        assert np.all(r > 1e-8)  # the generator keeps every view off the principal axis
        ir = 1 / r
        dthd = 1 + 3 * v[4] * th ** 2 + 5 * v[5] * th ** 4 + 7 * v[6] * th ** 6 + 9 * v[7] * th ** 8
        dth_dr = 1 / (r * r + 1)
        # duv_dxy (dxy_dxyn + (dxy_dr + dxy_dthd dthd_dth dth_dr) dr_dxyn)
        a = np.stack([-x * thd * ir * ir + x * ir * dthd * dth_dr, -y * thd * ir * ir + y * ir * dthd * dth_dr], 1)
        b = np.stack([x * ir, y * ir], 1)
        M = a[:, :, None] * b[:, None, :]
        M[:, 0, 0] += thd * ir
        M[:, 1, 1] += thd * ir
        dzn[:, 0, :] = v[0] * M[:, 0, :]
        dzn[:, 1, :] = v[1] * M[:, 1, :]
        cd = thd * ir
        dze[:, 0, 0], dze[:, 0, 2] = x * cd, 1
        dze[:, 1, 1], dze[:, 1, 3] = y * cd, 1
        for k, p in enumerate((3, 5, 7, 9)):
            dze[:, 0, 4 + k] = v[0] * x * ir * th ** p
            dze[:, 1, 4 + k] = v[1] * y * ir * th ** p
    return dzn, dze


# ---------------------------------------------------------------------------------------------------------------
# a feature: its measurements in the caller's order
Feat = namedtuple("Feat", "fid cam clone uv uvn kind")  # cam, clone: int arrays; uv, uvn: float32 (m, 2)


def anchor_of(f):
    """single_triangulation's anchor (FeatureInitializer.cpp:33-47): the camera with the most measurements, the first
    such in the iteration order of Feature::timestamps, and that camera's last clone.  The map is a libstdc++
    unordered_map with a handful of integer keys: it iterates in reverse order of insertion."""
    order = camera_order(f)
    best, n = order[0], 0
    for c in order:
        k = int(np.sum(f.cam == c))
        if k > n:
            best, n = c, k
    return best, int(f.clone[f.cam == best][-1])


def camera_order(f):
    seen = []
    for c in f.cam:
        if int(c) not in seen:
            seen.append(int(c))
    return seen[::-1]


def reference_rows(f):
    """the measurement indices in the order the reference's rows come: camera by camera (camera_order), each
    camera's in observation order"""
    return np.concatenate([np.nonzero(f.cam == c)[0] for c in camera_order(f)])


Lin = namedtuple("Lin", "res H_f H_x cols casts")


def feature_jacobian(st, f, rep, do_fej, p_FinG=None, p_FinA=None, anchor=None, dt=LD, inject=None):
    """res (2m), H_f (2m, 3), H_x (2m, len(cols)) and the covariance id of every column, rows in the order of the
    feature's measurements.  rep 0 takes p_FinG; rep 4 takes p_FinA in the anchor (cam, clone) frame, or p_FinG, from
    which p_FinA follows through the anchor's current pose.  inject (tests of the tests): "clone_pos_sign" flips
    the sign of the clone position block, "swap_fej" linearizes at the other of the two estimates."""
    assert rep in (0, 4)
    if inject == "swap_fej":
        do_fej = not do_fej
    m = len(f.cam)
    casts = Casts()
    one = np.eye(3, dtype=dt)
    if rep == 4:
        ac, ai = anchor if anchor is not None else anchor_of(f)
        Rca, pca = st.extrinsic(ac, dt)
        Ra, pa = st.clone(ai, False, dt)
        if p_FinA is None:
            p_FinA = Rca @ (Ra @ (np.asarray(p_FinG, dtype=dt) - pa)) + pca
        p_FinA = np.asarray(p_FinA, dtype=dt)
        p_FinG = Ra.T @ (Rca.T @ (p_FinA - pca)) + pa  # UpdaterHelper.cpp:271-283
    p_FinG = np.asarray(p_FinG, dtype=dt)
    # columns: the measured clones, the cameras' calibration, the anchor's
    cols, at = [], {}

    def block(key, cid, size):
        if key not in at:
            at[key] = len(cols)
            cols.extend(range(cid, cid + size))
        return at[key]

    for j in range(m):
        block(("clone", int(f.clone[j])), st.clones[int(f.clone[j])][0], 6)
        if st.calib_ext:
            block(("ext", int(f.cam[j])), st.ext[int(f.cam[j])][0], 6)
        if st.calib_intr:
            block(("intr", int(f.cam[j])), st.intr[int(f.cam[j])][0], 8)
    if rep == 4:
        block(("clone", ai), st.clones[ai][0], 6)
        if st.calib_ext:
            block(("ext", ac), st.ext[ac][0], 6)
    # the representation (UpdaterHelper.cpp:32-190)
    dl, H_anc, H_cal = one, None, None
    if rep == 4:
        R_GtoI, p_IinG, pA = Ra, pa, p_FinA
        if do_fej:
            R_GtoI, p_IinG = st.clone(ai, True, dt)
            pA = (R_GtoI.T @ Rca.T).T @ (p_FinG - p_IinG) + pca
        R_CtoG = R_GtoI.T @ Rca.T
        H_anc = np.concatenate([-(R_GtoI.T @ skew(Rca.T @ (pA - pca), dt)), one], axis=1)
        H_cal = np.concatenate([-(R_CtoG @ skew(pA - pca, dt)), -R_CtoG], axis=1)
        alpha, beta, rho = pA[0] / pA[2], pA[1] / pA[2], 1 / pA[2]
        d = np.zeros((3, 3), dtype=dt)
        d[0, 0] = d[1, 1] = 1 / rho
        d[0, 2], d[1, 2], d[2, 2] = -(1 / (rho * rho)) * alpha, -(1 / (rho * rho)) * beta, -(1 / (rho * rho))
        dl = R_CtoG @ d
    # the measurement model, all measurements at once (UpdaterHelper.cpp:310-404)
    Rc = np.stack([st.clone(int(i), False, dt)[0] for i in f.clone])
    pc = np.stack([st.clone(int(i), False, dt)[1] for i in f.clone])
    RIC = np.stack([st.extrinsic(int(c), dt)[0] for c in f.cam])
    pIC = np.stack([st.extrinsic(int(c), dt)[1] for c in f.cam])
    zeta = np.stack([st.intrinsics(int(c), dt) for c in f.cam])
    p_I = np.einsum("mij,mj->mi", Rc, p_FinG[None, :] - pc)
    p_C = np.einsum("mij,mj->mi", RIC, p_I) + pIC
    xn, yn = p_C[:, 0] / p_C[:, 2], p_C[:, 1] / p_C[:, 2]
    xf, yf = casts.f32(xn), casts.f32(yn)
    res = np.zeros(2 * m, dtype=dt)
    dzn, dze = np.zeros((m, 2, 2), dtype=dt), np.zeros((m, 2, 8), dtype=dt)
    for c in set(int(c) for c in f.cam):
        k = np.nonzero(f.cam == c)[0]
        model, v = st.cams[c].model, zeta[k[0]]
        u, w = distort(model, v, xf[k], yf[k], dt)
        uf, wf = casts.f32(u), casts.f32(w)
        res[2 * k] = f.uv[k, 0].astype(dt) - uf.astype(dt)
        res[2 * k + 1] = f.uv[k, 1].astype(dt) - wf.astype(dt)
        dzn[k], dze[k] = distort_jacobian(model, v, xn[k], yn[k], dt)  # at the current (xn, yn), FEJ or not
    if do_fej:
        Rc = np.stack([st.clone(int(i), True, dt)[0] for i in f.clone])
        pc = np.stack([st.clone(int(i), True, dt)[1] for i in f.clone])
        p_I = np.einsum("mij,mj->mi", Rc, p_FinG[None, :] - pc)  # p_FinG_fej is p_FinG (UpdaterMSCKF.cpp:169-178)
        p_C = np.einsum("mij,mj->mi", RIC, p_I) + pIC
    dzn_dpfc = np.zeros((m, 2, 3), dtype=dt)
    dzn_dpfc[:, 0, 0] = dzn_dpfc[:, 1, 1] = 1 / p_C[:, 2]
    dzn_dpfc[:, 0, 2] = -p_C[:, 0] / (p_C[:, 2] * p_C[:, 2])
    dzn_dpfc[:, 1, 2] = -p_C[:, 1] / (p_C[:, 2] * p_C[:, 2])
    dpfc_dpfg = RIC @ Rc
    sgn = -1 if inject == "clone_pos_sign" else 1
    dpfc_dclone = np.concatenate([RIC @ skew_b(p_I), -sgn * dpfc_dpfg], axis=2)
    dz_dpfc = dzn @ dzn_dpfc
    dz_dpfg = dz_dpfc @ dpfc_dpfg
    H_f = (dz_dpfg @ dl).reshape(2 * m, 3)
    H_x = np.zeros((2 * m, len(cols)), dtype=dt)
    Hc = dz_dpfc @ dpfc_dclone
    if st.calib_ext:
        He = dz_dpfc @ np.concatenate([skew_b(p_C - pIC), np.broadcast_to(one, (m, 3, 3))], axis=2)
    for j in range(m):
        r = slice(2 * j, 2 * j + 2)
        o = at[("clone", int(f.clone[j]))]
        H_x[r, o:o + 6] = Hc[j]
        if rep == 4:
            o = at[("clone", ai)]
            H_x[r, o:o + 6] += dz_dpfg[j] @ H_anc
            if st.calib_ext:
                o = at[("ext", ac)]
                H_x[r, o:o + 6] += dz_dpfg[j] @ H_cal
        if st.calib_ext:
            o = at[("ext", int(f.cam[j]))]
            H_x[r, o:o + 6] += He[j]
        if st.calib_intr:
            o = at[("intr", int(f.cam[j]))]
            H_x[r, o:o + 8] = dze[j]
    return Lin(res, H_f, H_x, np.array(cols, dtype=np.intp), casts)


def nullspace_project(H_f, H_x, res):
    """[H_x | res] with H_f's column space projected out: three Householder reflections, the first three rows dropped"""
    dt = H_f.dtype
    Hf = np.array(H_f)
    A = np.concatenate([H_x, res[:, None]], axis=1)
    for c in range(Hf.shape[1]):
        x = Hf[c:, c]
        nx = np.sqrt(x @ x)
        if nx == 0:
            continue
        v = np.array(x)
        v[0] -= -nx if x[0] > 0 else nx
        beta = dt.type(2) / (v @ v)
        Hf[c:, c:] -= beta * np.outer(v, v @ Hf[c:, c:])
        A[c:] -= beta * np.outer(v, v @ A[c:])
    k = Hf.shape[1]
    return A[k:, :-1], A[k:, -1]


def chi2_of(P, cols, H, res, sigma2):
    """res^T (H P[cols, cols] H^T + sigma2 I)^-1 res"""
    dt = H.dtype
    Pm = np.asarray(P, dtype=dt)[np.ix_(cols, cols)]
    S = H @ Pm @ H.T
    S = (S + S.T) / 2 + dt.type(sigma2) * np.eye(S.shape[0], dtype=dt)
    if dt == LD:
        y = fwd_ld(chol_ld(S), res)
    else:
        y = np.linalg.solve(np.linalg.cholesky(S), res)
    return y @ y


Eval = namedtuple("Eval", "chi2 rows P_plus dx x_plus casts idx H res")


def evaluate(st, feats, p_FinG, accepted, rep, do_fej, sigma2, dt=LD, inject=None):
    """The batch at the given landmark positions: chi2 of every feature with a position (p_FinG[i] is None for one
    that was not triangulated), and the update of the state by the features `accepted` (indices).
    casts[i]: the feature's smallest midpoint distance."""
    chi2, rows, casts, blocks = {}, {}, {}, []
    for i, f in enumerate(feats):
        if p_FinG[i] is None:
            continue
        lin = feature_jacobian(st, f, rep, do_fej, p_FinG=p_FinG[i], dt=dt, inject=inject)
        H, r = nullspace_project(lin.H_f, lin.H_x, lin.res)
        chi2[i] = chi2_of(st.P, lin.cols, H, r, sigma2)
        rows[i] = H.shape[0]
        casts[i] = lin.casts.dist
        if i in accepted:
            blocks.append((lin.cols, H, r))
    if not blocks:
        return Eval(chi2, rows, None, None, None, casts, None, None, None)
    idx = []
    for cols, _, _ in blocks:
        idx.extend(int(c) for c in cols if int(c) not in idx)
    # (membership in a list: a few hundred columns at most)
    pos = {c: k for k, c in enumerate(idx)}
    m = sum(b[1].shape[0] for b in blocks)
    Hb, rb = np.zeros((m, len(idx)), dtype=dt), np.zeros(m, dtype=dt)
    at = 0
    for cols, H, r in blocks:
        Hb[at:at + H.shape[0], [pos[int(c)] for c in cols]] = H
        rb[at:at + H.shape[0]] = r
        at += H.shape[0]
    if dt == LD:
        Pp, dx = ekf_update_ref(st.P, idx, Hb, rb, sigma2)
    else:
        Pp, dx = update_f64(st.P, idx, Hb, rb, sigma2)
    xp = boxplus(st.val, st.meta, dx, dt)
    return Eval(chi2, rows, Pp, dx, xp, casts, np.array(idx), Hb, rb)


def update_f64(P, idx, H, res, sigma2):
    """StateHelper::EKFUpdate in float64, the plain way (the second yardstick: what double precision alone costs)"""
    P = np.asarray(P, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.intp)
    T = H @ P[idx, :]
    S = T[:, idx] @ H.T
    S = (S + S.T) / 2 + sigma2 * np.eye(H.shape[0])
    L = np.linalg.cholesky(S)
    Wt = np.linalg.solve(L, T)
    return P - Wt.T @ Wt, Wt.T @ np.linalg.solve(L, res)


# ---------------------------------------------------------------------------------------------------------------
Tri = namedtuple("Tri", "cond depth ratio p_FinA p_FinG anchor")


def triangulate_linear(st, f, dt=LD):
    """FeatureInitializer::single_triangulation: the solution, cond(A) = its largest over its smallest singular
    value (A is symmetric positive semidefinite: its eigenvalues, in float64), the depth p_FinA[2], and the baseline
    ratio |p_FinA| / max_i |p_CiinA perpendicular to p_FinA| that single_gaussnewton tests after its refinement"""
    ac, ai = anchor_of(f)
    R_GtoA, p_AinG = st.cam_pose(ai, ac, dt)
    A, b, pcs = np.zeros((3, 3), dtype=dt), np.zeros(3, dtype=dt), []
    for j in range(len(f.cam)):
        R_GtoC, p_CinG = st.cam_pose(int(f.clone[j]), int(f.cam[j]), dt)
        R_AtoC = R_GtoC @ R_GtoA.T
        p_CinA = R_GtoA @ (p_CinG - p_AinG)
        bi = R_AtoC.T @ np.array([f.uvn[j, 0], f.uvn[j, 1], 1], dtype=dt)
        bi = bi / np.sqrt(bi @ bi)
        B = skew(bi, dt)
        Ai = B.T @ B
        A += Ai
        b += Ai @ p_CinA
        pcs.append(p_CinA)
    w = np.linalg.eigvalsh(A.astype(np.float64))
    cond = float(w[-1] / w[0]) if w[0] > 0 else float("inf")
    if not np.isfinite(cond) or cond > 1e12:
        return Tri(cond, float("nan"), float("nan"), None, None, (ac, ai))
    L = chol_ld(A)
    p = fwd_ld(L, b)
    for i in range(2, -1, -1):  # L^T p = y, in place
        p[i] = (p[i] - L[i + 1:, i] @ p[i + 1:]) / L[i, i]
    p = p.astype(dt)
    if not p @ p > 0:  # every view from the anchor's own pose: b = 0
        return Tri(cond, float(p[2]), float("inf"), p, R_GtoA.T @ p + p_AinG, (ac, ai))
    vh = p / np.sqrt(p @ p)
    base = max(float(np.sqrt((q - (q @ vh) * vh) @ (q - (q @ vh) * vh))) for q in pcs)
    ratio = float(np.sqrt(p @ p)) / base if base > 0 else float("inf")
    return Tri(cond, float(p[2]), ratio, p, R_GtoA.T @ p + p_AinG, (ac, ai))


# ---------------------------------------------------------------------------------------------------------------
# the generator
def make_state(val, meta, clone_times, cams, calib_ext, calib_intr, seed, span=(-5.0, -2.0)):
    """The given layout with fej = val boxplus a fixed perturbation of 1e-3 on the clones and the extrinsics, and a
    covariance graded as ekf_ref.graded_case grades it: P = D (A A^T / N + 1e-3 I) D, D a random permutation of
    logspace(span) (standard deviations from 1e-5 to 1e-2: with 1 px of noise on consistent measurements an
    accepted batch then moves no state component by 0.1, tests/test_feat_ref.py checks it, and a 50 px outlier stays
    far outside what H P H^T explains)."""
    st = State(val, val, meta, np.eye(1), clone_times, cams, calib_ext, calib_intr)
    rng = np.random.default_rng(seed)
    N = st.N
    d = np.zeros(N)
    for cid, _ in st.clones + (st.ext or []):
        d[cid:cid + 6] = 1e-3 * rng.standard_normal(6)
    fej = boxplus(st.val, st.meta, d, LD).astype(np.float64)
    D = np.logspace(span[0], span[1], N)[rng.permutation(N)]
    A = rng.standard_normal((N, N))
    P = (A @ A.T / N + 1e-3 * np.eye(N)) * np.outer(D, D)
    P = np.triu(P) + np.triu(P, 1).T
    return State(val, fej, meta, P, clone_times, cams, calib_ext, calib_intr)


def views_of(kind, m, K, C):
    """the (clone, camera) pairs of a feature of this kind: accepted features and outliers are spread over the window
    (views), the two triangulation rejections have the views their construction needs (_cond_views, _depth_views)"""
    if kind == "cond":
        return [(K - 1, 0)] * max(m, 2)
    if kind == "depth":  # (the two far clones are chosen on the state; every case that has this feature also has one
        return [(0, 0), (K // 2 - 1, 0), (K - 1, 0), (K // 2, 0)]  # over all clones, so the batch's columns stay)
    return views(m, K, C)


def views(m, K, C):
    """m distinct (clone, camera) pairs spread over the K x C there are, in observation order (time, then camera)"""
    assert 2 <= m <= K * C
    k = np.unique(np.round(np.linspace(0, K * C - 1, m)).astype(int))
    assert len(k) == m
    return [(int(i) // C, int(i) % C) for i in k]


def columns_of(st, vw):
    """the state columns a feature with these views touches under rep 0 (its nf in k_feature)"""
    n = 6 * len(set(i for i, _ in vw))
    cams = set(c for _, c in vw)
    return n + (6 * len(cams) if st.calib_ext else 0) + (8 * len(cams) if st.calib_intr else 0)


def project(st, i, c, p_FinG):
    """the exact (longdouble) pixel of p_FinG in camera c at clone i, and its depth"""
    RG, pG = st.cam_pose(i, c, LD)
    p = RG @ (np.asarray(p_FinG, dtype=LD) - pG)
    v = st.intrinsics(c, LD)
    x, y = p[0] / p[2], p[1] / p[2]
    r = np.sqrt(x * x + y * y)
    if st.cams[c].model == 0:
        r2 = r * r
        x1 = x * (1 + v[4] * r2 + v[5] * r2 * r2) + 2 * v[6] * x * y + v[7] * (r2 + 2 * x * x)
        y1 = y * (1 + v[4] * r2 + v[5] * r2 * r2) + v[6] * (r2 + 2 * y * y) + 2 * v[7] * x * y
    else:
        th = np.arctan(r)
        cd = (th + v[4] * th ** 3 + v[5] * th ** 5 + v[6] * th ** 7 + v[7] * th ** 9) / r
        x1, y1 = x * cd, y * cd
    return np.array([v[0] * x1 + v[2], v[1] * y1 + v[3]], dtype=LD), p[2]


def _visible(st, vw, p):
    px = []
    for i, c in vw:
        uv, z = project(st, i, c, p)
        cam = st.cams[c]
        if not (z > 0.3 and 25 < uv[0] < cam.width - 25 and 25 < uv[1] < cam.height - 25):
            return None
        px.append(uv)
    return np.array(px)


def _landmark(st, vw, rng, depth_max):
    """a landmark seen by every view: on a ray through the middle view, at a log-uniform depth in
    [0.5, min(40, depth_max)] m"""
    i, c = vw[len(vw) // 2]
    cam = st.cams[c]
    v = cam.intrinsics
    RG, pG = st.cam_pose(i, c, LD)
    for _ in range(400):
        u = rng.uniform(0.25, 0.75) * cam.width, rng.uniform(0.25, 0.75) * cam.height
        d = float(np.exp(rng.uniform(np.log(0.5), np.log(min(40.0, max(depth_max, 0.6))))))
        ray = np.array([(u[0] - v[2]) / v[0], (u[1] - v[3]) / v[1], 1.0])
        if np.hypot(ray[0], ray[1]) < 0.02:
            continue
        p = pG + RG.T @ (ray.astype(LD) * d)
        px = _visible(st, vw, p)
        if px is not None:
            return p, px
    raise AssertionError("no landmark is visible from all of %s" % (vw,))


def _baseline(st, vw):
    c = [np.asarray(st.cam_pose(i, k, np.float64)[1]) for i, k in vw]
    return max(np.linalg.norm(a - b) for a in c for b in c)


def _feature(fid, vw, px, undistort, kind):
    cam = np.array([c for _, c in vw], dtype=np.int64)
    clone = np.array([i for i, _ in vw], dtype=np.int64)
    uv = np.asarray(px, dtype=LD).astype(F32)
    uvn = np.zeros_like(uv)
    for c in set(int(c) for c in cam):
        k = np.nonzero(cam == c)[0]
        uvn[k] = undistort(c, uv[k])
    return Feat(fid, cam, clone, uv, uvn, kind)


def _ok_views(st, m, rng, undistort, fid, sigma2, rep, do_fej, kind="ok", vw=None):
    """an m-measurement feature with 1 px of noise whose chi2, taken at the linear triangulation, is below a third
    of its threshold (the noise is redrawn otherwise; the tests hold the actual chi2 to a margin of 2).  With
    sigma_pix = 1 a feature of many rows has chi2 near its row count R, which no threshold chi2_95(R) exceeds by a
    factor of 2: there the noise is sqrt(chi2_95(R) / (3 R)) px (0.8 px at 9 rows, 0.64 px at 125)."""
    K, C = len(st.clone_times), len(st.cams)
    vw = views(m, K, C) if vw is None else vw
    noise = min(1.0, (chi2_95(rows_of(m)) / (3.0 * rows_of(m) * sigma2)) ** 0.5 * sigma2 ** 0.5)
    depth_max = 8.0 * _baseline(st, vw)  # |p_FinA| / baseline <= fi_max_baseline / 4, roughly
    for _ in range(60):
        p, px = _landmark(st, vw, rng, depth_max)
        f = _feature(fid, vw, px + noise * rng.standard_normal(px.shape), undistort, kind)
        t = triangulate_linear(st, f, np.float64)
        if t.p_FinG is None or not (t.cond < 2000 and 0.4 < t.depth < 25 and t.ratio < 12):
            continue
        lin = feature_jacobian(st, f, rep, do_fej, p_FinG=t.p_FinG, dt=np.float64)
        H, r = nullspace_project(lin.H_f, lin.H_x, lin.res)
        if chi2_of(st.P, lin.cols, H, r, sigma2) < chi2_95(H.shape[0]) / 3:
            return f
    raise AssertionError("no accepted feature of %d measurements" % m)


def _cond_views(st, m, rng, undistort, fid):
    """status 1: m views of one landmark from ONE camera pose (the last clone, camera 0), 0.1 px of noise apart: the
    rays meet in the camera centre, A has one direction a factor of about (0.1 px / focal length)^2 below the others"""
    vw = views_of("cond", m, len(st.clone_times), len(st.cams))
    p, px = _landmark(st, vw[:1], rng, 10.0)
    return _feature(fid, vw, np.repeat(px, len(vw), 0) + 0.1 * rng.standard_normal((len(vw), 2)), undistort, "cond")


def _depth_views(st, rng, undistort, fid, fi_max_dist):
    """status 2: four views of camera 0, no noise.  The anchor is the middle clone (its measurement is listed last:
    the anchor is the last measurement of the camera with the most, FeatureInitializer.cpp:33-47).  A view one clone
    away (baseline b1) agrees with the depth z1 on the anchor's ray; the first and the last clone (baselines b2, b3
    on either side) agree with an infinite depth.  The linear solution weighs every ray by metric distance: the two
    parallel rays hold the point near the anchor's ray and the near view puts it at about z1.  The refinement
    weighs errors in the normalized image plane, in which every view's error shrinks with the inverse depth rho:
    b1^2 (1 / z1 - rho)^2 + (b2^2 + b3^2) rho^2 has its minimum at the depth z1 (1 + (b2^2 + b3^2) / b1^2), and z1 is
    held to at least 4 fi_max_dist here.  Only the near view fixes the depth of the linear solution, whose condition
    number is 5 to 12 (z1 / b1)^2: with z1 of 0.3 to 0.5 m it stays below fi_max_cond_number / 2 because the near
    view is the window's one short step (CLONE_SHORT_GAP).  The linear solution is held to margins inside those
    the tests ask for."""
    K = len(st.clone_times)
    mid = K // 2
    near = mid - 1
    centre = [np.asarray(st.cam_pose(i, 0, np.float64)[1]) for i in range(K)]
    base = [float(np.linalg.norm(c - centre[mid])) for c in centre]
    b1 = base[near]
    cam = st.cams[0]
    v = cam.intrinsics
    RG, pG = st.cam_pose(mid, 0, LD)
    # the far views: among the outermost clones the pair most equal in baseline (b2 - b3 moves the linear solution
    # sideways and so along the near view's ray, away from z1)
    pairs = sorted((abs(base[i] - base[j]), i, j) for i in range(min(3, near)) for j in range(max(K - 3, mid + 1), K))
    for _, far0, far1 in pairs:
        vw = [(far0, 0), (near, 0), (far1, 0), (mid, 0)]
        gain = 1 + (base[far0] ** 2 + base[far1] ** 2) / (b1 * b1)
        for z1 in (0.5, 0.42, 0.35, 0.3):
            if z1 * gain < 4 * fi_max_dist:
                continue
            for _ in range(40):
                u = rng.uniform(0.15, 0.85) * cam.width, rng.uniform(0.15, 0.85) * cam.height
                ray = (RG.T @ np.array([(u[0] - v[2]) / v[0], (u[1] - v[3]) / v[1], 1.0], dtype=LD))
                near_p, far_p = pG + ray * z1, pG + ray * 1e7
                px = [_visible(st, vw[0:1], far_p), _visible(st, vw[1:2], near_p), _visible(st, vw[2:3], far_p),
                      _visible(st, vw[3:4], near_p)]
                if any(q is None for q in px):
                    continue
                f = _feature(fid, vw, np.concatenate(px), undistort, "depth")
                t = triangulate_linear(st, f, np.float64)
                if t.p_FinG is not None and t.cond < 4500 and 0.22 < t.depth < fi_max_dist / 2.5:
                    return f
    raise AssertionError("no view set for the depth rejection")


def _outlier_views(st, m, rng, undistort, fid, sigma2, rep, do_fej):
    """status 3: an accepted feature with one measurement moved by 50 px, across the direction in which the
    landmark's pixel travels over the views: the triangulated depth hardly moves, so the feature still passes the
    triangulation (its linear quantities are held to the accepted features' margins) and reaches the gate"""
    for _ in range(20):
        f = _ok_views(st, m, rng, undistort, fid, sigma2, rep, do_fej)
        uv = np.array(f.uv)
        j = len(uv) // 2
        cam = st.cams[int(f.cam[j])]
        same = np.nonzero(f.cam == f.cam[j])[0]
        assert len(same) >= 2
        travel = uv[same[-1]].astype(np.float64) - uv[same[0]].astype(np.float64)
        across = np.array([-travel[1], travel[0]]) / max(np.hypot(*travel), 1e-9)
        for sign in (1.0, -1.0):
            moved = uv[j].astype(np.float64) + sign * 50.0 * across
            if not (25 < moved[0] < cam.width - 25 and 25 < moved[1] < cam.height - 25):
                continue
            out = np.array(uv)
            out[j] = moved.astype(F32)
            g = _feature(fid, list(zip(f.clone.tolist(), f.cam.tolist())), out, undistort, "outlier")
            t = triangulate_linear(st, g, np.float64)
            if t.p_FinG is not None and t.cond < 2000 and 0.4 < t.depth < 25 and t.ratio < 12:
                return g
    raise AssertionError("no outlier feature of %d measurements" % m)


STATUS = {"ok": 0, "cond": 1, "depth": 2, "outlier": 3}


def chi2_95(dof):
    """boost::math::quantile(chi_squared(dof), 0.95) by Newton on the regularized gamma function's series (float64;
    the tests compare it with the oracle's table)"""
    from math import exp, lgamma, log
    a = dof / 2.0

    def cdf(x):  # P(a, x / 2)
        z = x / 2.0
        if z < a + 1:
            t = s = 1.0 / a
            k = a
            while abs(t) > 1e-17 * abs(s):
                k += 1
                t *= z / k
                s += t
            return s * exp(-z + a * log(z) - lgamma(a))
        b = z + 1 - a  # continued fraction of Q (Lentz)
        c, d = 1e300, 1.0 / b
        h = d
        for i in range(1, 500):
            an = -i * (i - a)
            b += 2
            d = an * d + b
            d = 1e-300 if abs(d) < 1e-300 else d
            c = b + an / c
            c = 1e-300 if abs(c) < 1e-300 else c
            d = 1.0 / d
            h *= d * c
            if abs(d * c - 1) < 1e-16:
                break
        return 1 - exp(-z + a * log(z) - lgamma(a)) * h

    x = dof * (1 - 2.0 / (9 * dof) + 1.6448536269514722 * (2.0 / (9 * dof)) ** 0.5) ** 3  # Wilson-Hilferty
    for _ in range(50):
        pdf = exp((a - 1) * log(x / 2) - x / 2 - lgamma(a)) / 2
        step = (cdf(x) - 0.95) / pdf
        x -= step
        if abs(step) < 1e-13 * x:
            break
    return x


def make_case(st, case, undistort, opts):
    """the features of a case (CASES entry) on the state st: [Feat]; opts gives sigma, the gate and the
    triangulation thresholds (msckf_sigma_pix, fi_max_dist)"""
    rng = np.random.default_rng(case["seed"])
    s2 = float(opts.msckf_sigma_pix) ** 2
    rep, fej = case["rep"], bool(case["fej"])
    feats = []
    for k, (kind, m) in enumerate(case["feats"]):
        fid = 1000 + k
        if kind == "ok":
            feats.append(_ok_views(st, m, rng, undistort, fid, s2, rep, fej))
        elif kind == "cond":
            feats.append(_cond_views(st, m, rng, undistort, fid))
        elif kind == "depth":
            feats.append(_depth_views(st, rng, undistort, fid, float(opts.fi_max_dist)))
        else:
            feats.append(_outlier_views(st, m, rng, undistort, fid, s2, rep, fej))
    clones = set(int(i) for f in feats if f.kind != "depth" for i in f.clone)
    assert all(set(int(i) for i in f.clone) <= clones for f in feats if f.kind == "depth")
    return feats


def as_measurements(st, feats):
    """the features as msckf_update takes them: [(featid, [(cam, t, u, v, un, vn), ...])]"""
    return [(f.fid, [(int(f.cam[j]), st.clone_times[int(f.clone[j])], float(f.uv[j, 0]), float(f.uv[j, 1]),
                      float(f.uvn[j, 0]), float(f.uvn[j, 1])) for j in range(len(f.cam))]) for f in feats]


# ---- the setups and the case list ----
# name -> (config directory, option overrides, clones, clone spacing in seconds); cols = the state columns a
# feature over every clone and camera touches
SETUPS = {
    # equidistant camera, nothing calibrated
    "mono": ("tum_vi", dict(num_cameras=1, use_stereo=0, do_calib_camera_pose=0, do_calib_camera_intrinsics=0,
                            do_calib_camera_timeoffset=0), 6, 0.3),
    # EuRoC stereo (radtan), extrinsics, intrinsics and time offset calibrated
    "stereo": ("euroc_mav", dict(), 11, 0.1),
    # four cameras (radtan), extrinsics only: the one setup whose k_feature LDS holds a 64-measurement feature
    "quad": ("rpng_sim_uwb", dict(use_uwb=0, do_calib_imu_intrinsics=0, do_calib_imu_g_sensitivity=0,
                                  do_calib_camera_intrinsics=0, do_calib_camera_timeoffset=0), 16, 0.06),
}
CLONE_SHORT_GAP = 0.025  # seconds between the clones K / 2 - 1 and K / 2 (about 2.5 cm of baseline)


def clone_offsets(setup):
    """the clone times of a setup, in seconds after the start: its spacing, but one short step into the middle clone"""
    _, _, K, dt = SETUPS[setup]
    gaps = [dt] * K
    gaps[K // 2] = CLONE_SHORT_GAP
    return [float(v) for v in np.cumsum(gaps)]


SHAPE = {"mono": (6, 1, 0, 0), "stereo": (11, 2, 6, 8), "quad": (16, 4, 6, 0)}  # clones, cameras, ext, intr columns


def _ncols(setup, m):
    K, C, e, i = SHAPE[setup]
    vw = views(m, K, C)
    return 6 * len(set(a for a, _ in vw)) + (e + i) * len(set(c for _, c in vw))


def _fill(target, mmax):
    """feature sizes whose projected rows sum to target, as many of mmax measurements as fit"""
    big = rows_of(mmax)
    for k in range(target // big, -1, -1):
        rest = target - k * big
        if rest == 0:
            return [mmax] * k
        for cnt in (1, 2, 3):
            for combo in itertools.combinations_with_replacement(range(mmax, 1, -1), cnt):
                if sum(rows_of(m) for m in combo) == rest:
                    return [mmax] * k + list(combo)
    raise AssertionError((target, mmax))


def _lds_edge(setup):
    """the largest feature whose H, T and S fit k_chi2's LDS (chi2_lds_bytes <= kMaxDynLds, launch_chi2_batch) on
    this setup, or None when every feature the setup can hold fits"""
    K, C, _, _ = SHAPE[setup]
    top = min(K * C, K_MAX_MEAS_PER_FEAT)
    fits = [m for m in range(2, top + 1) if chi2_lds_bytes(rows_of(m), _ncols(setup, m)) <= K_MAX_DYN_LDS]
    return None if fits[-1] == top else fits[-1]


def _cases():
    out = []
    seed = [4000]

    def add(setup, name, feats, fej=1, rep=0):
        seed[0] += 1
        out.append(dict(id="%s-%s-fej%d-rep%d" % (setup, name, fej, rep), setup=setup, fej=fej, rep=rep,
                        feats=[(k, int(m)) for k, m in feats], seed=seed[0]))

    ok = lambda *ms: [("ok", m) for m in ms]  # noqa: E731
    # (the mono window of 6 clones does not give the status-2 construction its margins: there the refinement ends
    # at 0.08 m, out of range by a factor 1.2 only; the other two setups carry that rejection)
    rejected = lambda setup: ([("cond", 4)] + ([("depth", 4)] if setup != "mono" else []) +  # noqa: E731
                              [("outlier", SHAPE[setup][0])])
    # -- mono: 6 clones, 36 columns: the smallest features, both sides of m = n, the rejections
    n = _ncols("mono", 6)
    for fej, rep in ((1, 0), (0, 4)):
        add("mono", "one2", ok(2), fej, rep)   # 1 projected row
        add("mono", "one3", ok(3), fej, rep)   # 3 projected rows
        add("mono", "rows=n", ok(*_fill(n, 6)), fej, rep)          # m <= n: the direct update, Tall reused
        add("mono", "rows=n+1", ok(*_fill(n + 1, 6)), fej, rep)    # m = n + 1: Gram and information form
        add("mono", "rejected", rejected("mono"), fej, rep)
        add("mono", "mixed", [("ok", 6), ("cond", 4), ("ok", 4), ("ok", 5), ("outlier", 6), ("ok", 3)], fej, rep)
    # -- stereo: 11 clones x 2 cameras, every calibration: 15 / 17 rows around a 16-row tile, the feature counts at
    # which the batch build changes (K_CHUNKED_BUILD)
    for fej, rep in ((1, 0), (0, 0), (1, 4)):
        add("stereo", "one9", ok(9), fej, rep)
        add("stereo", "one10", ok(10), fej, rep)
        add("stereo", "sizes", ok(2, 3, 9, 10, 22), fej, rep)
        add("stereo", "mixed",
            [("ok", 9), ("outlier", 8), ("ok", 3), ("cond", 5), ("ok", 22), ("depth", 4), ("ok", 10)],
            fej, rep)
    add("stereo", "rejected", rejected("stereo"))
    for nfeat in (K_CHUNKED_BUILD - 1, K_CHUNKED_BUILD, K_CHUNKED_BUILD + 1):
        add("stereo", "n%d" % nfeat, ok(*[2 + (k % 3) for k in range(nfeat)]))
    # -- quad: 16 clones x 4 cameras, extrinsics: the large features
    edge = _lds_edge("quad")
    assert edge is not None and _lds_edge("mono") is None and _lds_edge("stereo") is None
    two = min(m for m in range(2, 65) if chi2_instance(rows_of(m)) == 2)  # the first k_chi2<2> feature
    sizes = sorted(set([33, 34, 64, edge, edge + 1, two - 1, two]))
    for m in sizes:
        add("quad", "one%d" % m, ok(m))
    add("quad", "one%d" % K_MAX_MEAS_PER_FEAT, ok(K_MAX_MEAS_PER_FEAT), 1, 4)
    add("quad", "one%d" % edge, ok(edge), 0, 4)
    big = rows_of(K_MAX_MEAS_PER_FEAT)
    add("quad", "rows%d" % (K_TILED_ROWS - 1), ok(*_fill(K_TILED_ROWS - 1, K_MAX_MEAS_PER_FEAT)))
    add("quad", "rows%d" % (-(-K_TILED_ROWS // big) * big), ok(*[K_MAX_MEAS_PER_FEAT] * -(-K_TILED_ROWS // big)))
    add("quad", "mixed", [("ok", 64), ("cond", 6), ("ok", 33), ("outlier", 40), ("depth", 4), ("ok", 10)])
    return out


CASES = _cases()
# rep 0 against rep 1 (GLOBAL_FULL_INVERSE_DEPTH) spans the same left nullspace: one case, no reference involved
REP01_CASE = next(c for c in CASES if c["id"] == "stereo-sizes-fej1-rep0")


def case_id(c):
    return c["id"]


def dispatch_of(c):
    """dispatch() of a case: the batch's columns are those of all its features, rejected ones included (the host
    builds the batch before anything is triangulated)"""
    K, C, e, i = SHAPE[c["setup"]]
    vw = [views_of(k, m, K, C) for k, m in c["feats"]]
    n = 6 * len(set(a for v in vw for a, _ in v)) + (e + i) * len(set(b for v in vw for _, b in v))
    return dispatch([len(v) for v in vw], n)


def dispatch_table():
    """one line per case: what dispatch() derives for it"""
    lines = []
    for c in CASES:
        d = dispatch_of(c)
        ms = [m for _, m in c["feats"]]
        lines.append("%-25s feats %3d max %2d rows %4d n %3d %-16s %-9s %-9s %-11s %s" %
                     (c["id"], len(ms), max(ms), d["rows"], d["n"], d["gemm"], d["chi2"], d["S"], d["update"],
                      d["build"]))
    return "\n".join(lines)


if __name__ == "__main__":
    print(dispatch_table())
