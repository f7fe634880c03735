"""Buffered pose fixes and the quaternion aux variable on the device: uvio_hp_feed_pose / uvio_hp_get_pose_results and
uvio_hp_aux_add_quat on a handle, and the chain's three kernels (k_pose_rows -> k_chain_M -> k_chain_update, the
6-row instances in FULL mode) on a standalone covariance (uvio_hp_debug_pose_update_p).

1. Numerics of the three kernels against the extended-precision reference (tests/pose_ref.py): N = 15, 16, 17, 33 (the
   edges of the 16-row tiles), ld = N and N + 5 (the padding comes back untouched), both modes, the lever arm and the
   mounting rotation each a constant, a state variable at 6 and one at N - 3 (the overlapping pairs left out).  P+
   exactly symmetric, and in ekf_ref.scaled_err / scaled_dx_err units
       e_dev <= RATIO * max(e_f64, 16 * 2^-52)
   with e_f64 the float64 NumPy comparator's error against the same reference.  RATIO = 4 x the worst measured ratio,
   rounded up to a power of two (the procedure of tests/test_gpu_meas_update.py).  Measured on MI355X over the 112
   cases (device error / max(float64 comparator's error, floor)):
       dx   5.69  N33-ld33-mode2-arm-1-rot-1  (device 2.02e-14, float64 3.34e-15: below the floor of 3.55e-15)
       P+   2.83  N17-ld17-mode2-arm6-rot-1   (device 1.71e-14, float64 6.02e-15)
   so RATIO = 32 (4 x 5.69 = 22.8).  The device forms the quaternion residual and H in another operation order than
   NumPy and sums S and W W^T with explicit FMAs; the residual carries an absolute rounding error of a few 2^-53
   whatever its size, and the largest ratios sit where the comparator's own error is at or below the floor.
   chi2 within 1e-10 (relative) of the reference's (measured: 6.2e-14 at worst), the gate applied on both sides of it.
2. An S that is not positive definite is refused with P unchanged; malformed arguments are refused before device work.
3. Buffered equals explicit: handle A queues an orientation fix and a full fix inside one frame interval, handle B does
   propagate + measurement_update with H and the residual from tests/pose_ref.py at B's state; state time and statuses
   equal, chi2 within 1e-10, x and P within the parity tests' 1e-10.
4. Two pose fixes at one timestamp: one chain, the second linearized at the state the first left.  Nine: two chains.
5. A pose fix, a position fix and a UWB message at one timestamp and at interleaved times against the explicit path.
6. An aux mounting rotation (and an aux lever arm) over three frames while clones are marginalized in front of them:
   the simulated sensor is turned 5 degrees from the initial q_ItoS, the estimate moves towards it and its marginal
   shrinks.  (With fixed camera intrinsics, as tests/test_gpu_position_feed.py's pair_fixed_intrinsics explains.)
7. The quaternion aux variable alone: append, boxplus, meta, walk, remove, an idle passenger, the norm refusal.
8. The C++ facade on the device (tests/cpp/facade_pose_check.cpp).
All inputs are consistent measurements or plainly malformed arguments.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import aux_ref as A  # noqa: E402
import ekf_ref as E  # noqa: E402
import meas_ref as M  # noqa: E402
import pose_ref as Q  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not E.HAVE_EXTENDED, reason=E.REASON)]

from test_gpu_meas_update import _rel, _true_range, _uwb_setup  # noqa: E402
from test_gpu_position_feed import (OVERRIDES, PRIOR3, R3, Pair, _explicit_fix, _imu_id,  # noqa: E402,F401
                                    _same_results, pair, pair_fixed_intrinsics, stream)

RATIO = 32.0
FLOOR = 16 * 2.0 ** -52
PAD = -7.25  # uvio_amd.manager._padded's filler
INF = float("inf")
# a mocap pose: 2 mrad and 3 mm, rotation and translation coupled
_D6 = np.array([2e-3, 2e-3, 2e-3, 3e-3, 3e-3, 3e-3])
_C6 = np.eye(6) + 0.2 * (np.eye(6, k=3) + np.eye(6, k=-3)) + 0.1 * (np.eye(6, k=1) + np.eye(6, k=-1))
R6 = _C6 * np.outer(_D6, _D6)
R3Q = R6[:3, :3].copy()
QS = M.quat_boxplus(np.array([0.0, 0.0, 0.0, 1.0]), np.array([0.3, -0.2, 0.5]))  # a mounting rotation of ~36 degrees
ARM = np.array([0.2, -0.05, 0.1])


def _blocks(N):
    return [(a, r) for a in (-1, 6, N - 3) for r in (-1, 6, N - 3) if a < 0 or a != r]


# ---- 1 ----
@pytest.mark.parametrize("N", [15, 16, 17, 33])
def test_three_kernels_against_extended_reference(N):
    import uvio_amd as U
    worst = {"P": (0.0, ""), "dx": (0.0, "")}
    for mode in (Q.ORIENTATION, Q.FULL):
        for ci, (arm_id, rot_id) in enumerate(_blocks(N)):
            k = Q.pose_case(N, mode, arm_id, rot_id, seed=12000 + 100 * N + 10 * ci + mode)
            args = (k.imu_id, k.q, k.p, k.s, k.qS, k.zq, k.zp, k.R, k.mode, k.arm_id, k.rot_id)
            Pr, dxr, c_ref = Q.pose_update_ref(k.P, *args)
            P6, dx6, _ = Q.pose_update_ref(k.P, *args, dtype=np.float64)
            c_ref = float(c_ref)
            e_64, x_64 = E.scaled_err(P6, Pr, k.P), E.scaled_dx_err(dx6, dxr, k.P)

            def run(ld, thr=INF):
                return U.pose_update_p(k.P, k.imu_id, k.q, k.p, k.s, k.qS, k.zq, k.R, z_p=k.zp, arm_id=arm_id,
                                       rot_id=rot_id, chi2_thr=thr, ld=ld)

            for ld in (N, N + 5):
                tag = "N%d-ld%d-mode%d-arm%d-rot%d" % (N, ld, mode, arm_id, rot_id)
                buf, dxg, chi2, applied = run(ld)
                Pg = buf[:, :N]
                e_dev, x_dev = E.scaled_err(Pg, Pr, k.P), E.scaled_dx_err(dxg, dxr, k.P)
                rp, rx = e_dev / max(e_64, FLOOR), x_dev / max(x_64, FLOOR)
                if rp > worst["P"][0]:
                    worst["P"] = (rp, "%s (device %.2e, float64 %.2e)" % (tag, e_dev, e_64))
                if rx > worst["dx"][0]:
                    worst["dx"] = (rx, "%s (device %.2e, float64 %.2e)" % (tag, x_dev, x_64))
                print("POSEPATH %s P dev %.3e f64 %.3e ratio %.2f dx dev %.3e f64 %.3e ratio %.2f chi2 rel %.2e" %
                      (tag, e_dev, e_64, rp, x_dev, x_64, rx, abs(chi2 - c_ref) / c_ref))
                assert applied and np.all(buf[:, N:] == PAD), tag
                assert np.array_equal(Pg, Pg.T), tag
                assert e_dev <= RATIO * max(e_64, FLOOR), (tag, e_dev, e_64)
                assert x_dev <= RATIO * max(x_64, FLOOR), (tag, x_dev, x_64)
                assert abs(chi2 - c_ref) < 1e-10 * c_ref, (tag, chi2, c_ref)
                # the gate on both sides of the reference's chi2
                b1, d1, c1, a1 = run(ld, c_ref * (1 + 1e-6))
                assert a1 and c1 == chi2 and np.array_equal(b1, buf) and np.array_equal(d1, dxg), tag
                b0, d0, c0, a0 = run(ld, c_ref * (1 - 1e-6))
                assert not a0 and c0 == chi2 and np.all(d0 == 0.0), tag
                assert np.array_equal(b0[:, :N], k.P) and np.all(b0[:, N:] == PAD), tag
    print("POSEWORST N%d P ratio %.2f %s | dx ratio %.2f %s" % (N, worst["P"][0], worst["P"][1], worst["dx"][0],
                                                                 worst["dx"][1]))


# ---- 2 ----
def test_standalone_refuses_an_indefinite_S_and_malformed_arguments():
    import uvio_amd as U
    k = Q.pose_case(17, Q.FULL, 6, 14, seed=43)
    _, H = Q.pose_model(k.q, k.p, k.s, k.qS, k.zq, k.zp, Q.FULL, True, True, np.float64)
    idx = Q.pose_columns(0, 6, 14, Q.FULL)
    big = 1e3 * np.max(np.abs(H @ k.P[np.ix_(idx, idx)] @ H.T))
    Rbad = big * (np.eye(6) + 10.0 * (np.ones((6, 6)) - np.eye(6)))  # a positive diagonal, far from positive definite

    def run(**over):
        kw = dict(P=k.P, imu_id=0, q=k.q, p=k.p, s=k.s, qS=k.qS, zq=k.zq, R=k.R, z_p=k.zp, arm_id=6, rot_id=14, thr=INF)
        kw.update(over)
        return U.pose_update_p(kw["P"], kw["imu_id"], kw["q"], kw["p"], kw["s"], kw["qS"], kw["zq"], kw["R"],
                               z_p=kw["z_p"], arm_id=kw["arm_id"], rot_id=kw["rot_id"], chi2_thr=kw["thr"])

    with pytest.raises(RuntimeError, match="E_ARG"):
        run(R=Rbad)
    buf, dx, chi2, applied = run()
    assert applied and not np.array_equal(buf, k.P)
    bad = [dict(arm_id=4), dict(rot_id=3), dict(rot_id=7), dict(arm_id=15), dict(rot_id=16), dict(imu_id=12),
           dict(zq=3.0 * k.zq), dict(zq=0.4 * k.zq), dict(qS=[0.0, 0.0, 0.0, 0.0]), dict(qS=[np.nan, 0.0, 0.0, 1.0]),
           dict(z_p=[np.inf, 0.0, 0.0]), dict(R=np.diag([1.0, 1.0, 0.0, 1.0, 1.0, 1.0])), dict(thr=0.0),
           dict(R=k.R[:, :5]), dict(p=[0.0, np.nan, 0.0]), dict(P=k.P[:8, :8])]
    for over in bad:
        with pytest.raises(RuntimeError, match="E_ARG"):
            run(**over)
    from uvio_amd import _native as N
    lib, dp = N.load(), C.POINTER(C.c_double)
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (k.P, k.q, k.p, k.s, k.qS, k.zq, k.zp, k.R, np.zeros(17))]
    P, q, p, s, qS, zq, zp, R, dx = [a.ctypes.data_as(dp) for a in arrs]
    chi2, app = C.c_double(), C.c_int()
    call = lib.uvio_hp_debug_pose_update_p
    assert call(P, 17, 17, 0, q, p, 6, s, 14, qS, 3, zq, zp, R, 6, INF, dx, C.byref(chi2), C.byref(app)) == N.E_ARG  # mode
    assert call(P, 17, 17, 0, q, p, 6, s, 14, qS, 2, zq, None, R, 6, INF, dx, C.byref(chi2), C.byref(app)) == N.E_ARG
    assert call(P, 17, 17, 0, q, p, 6, s, 14, qS, 2, zq, zp, R, 5, INF, dx, C.byref(chi2), C.byref(app)) == N.E_ARG
    assert np.array_equal(arrs[0], k.P)
    # the indefinite S again, through the C ABI: the refusal comes after the device work and P comes back unchanged
    Rb = np.ascontiguousarray(Rbad)
    assert call(P, 17, 17, 0, q, p, 6, s, 14, qS, 2, zq, zp, Rb.ctypes.data_as(dp), 6, INF, dx, C.byref(chi2),
                C.byref(app)) == N.E_ARG
    assert app.value == 0 and np.array_equal(arrs[0], k.P) and np.all(arrs[8] == 0.0)


# ---- the explicit path: propagate + measurement_update with tests/pose_ref.py's H and residual ----
def _pose_blocks(g, full, rot_h, arm_h):
    blocks = [(_imu_id(g), 6)]
    if arm_h and full:
        blocks.append((g.aux_state(arm_h)[0], 3))
    if rot_h:
        blocks.append((g.aux_state(rot_h)[0], 3))
    return blocks


def _explicit_pose(g, t, R, d=None, z=None, qS=QS, s=ARM, rot_h=0, arm_h=0, chi2_mult=1.0):
    """propagate to t (unless already there); the measurement is z = (z_q, z_p or None) or the prediction moved by the
    offset d (3: orientation only, 6: full); returns (z_q, z_p, result)"""
    import uvio_amd as U
    if g.get_imu_state()[0] < t:
        g.propagate(t)
    x = g.get_imu_state()[1]
    q, p = x[0:4], x[4:7]
    qSv = g.aux_state(rot_h)[1] if rot_h else np.asarray(qS, dtype=np.float64)
    sv = g.aux_state(arm_h)[1] if arm_h else np.asarray(s, dtype=np.float64)
    if z is None:
        d = np.asarray(d, dtype=np.float64)
        zq = M.quat_boxplus(M.quat_multiply(qSv, q), d[:3])
        zp = p + M.quat_2_Rot(q).T @ sv + d[3:] if d.size == 6 else None
    else:
        zq, zp = z
    full = zp is not None
    res, H = Q.pose_model(q, p, sv, qSv, zq, zp, Q.FULL if full else Q.ORIENTATION, arm_h > 0, rot_h > 0, np.float64)
    out = g.measurement_update(_pose_blocks(g, full, rot_h, arm_h), H, res, R, chi2_mult * U.chi2_95(6 if full else 3))
    return zq, zp, out


def _close(p, tag):
    xa, ma = p.ga.get_state_vector()
    xb, mb = p.gb.get_state_vector()
    assert p.ga.get_imu_state()[0] == p.gb.get_imu_state()[0]
    assert np.array_equal(ma, mb), "state layouts differ"
    ex, eP = _rel(xa, xb), _rel(p.ga.get_cov(), p.gb.get_cov())
    print("POSEPAIR %s x rel %.2e P rel %.2e" % (tag, ex, eP))
    assert ex < 1e-10 and eP < 1e-10, (tag, ex, eP)


# ---- 3 ----
def test_buffered_pose_fixes_equal_the_explicit_path(pair):
    ga, gb = pair.ga, pair.gb
    assert ga.pose_results() == []
    pair.feed_imu()
    ta, tb = pair.times(0.3, 0.65)
    za, _, oa = _explicit_pose(gb, ta, R3Q, d=[4e-3, -3e-3, 2e-3])
    zb, pb, ob = _explicit_pose(gb, tb, R6, d=[-3e-3, 2e-3, 3e-3, 0.006, -0.004, 0.005])
    assert oa["applied"] and ob["applied"], "a consistent pose was gated"
    assert ga.feed_measurement_pose(ta, za, R3Q, q_ItoS=QS)
    assert ga.feed_measurement_pose(tb, zb, R6, z_p=pb, q_ItoS=QS, p_SinI=ARM)
    assert not pair.identical()
    pair.frame()
    _same_results(ga.pose_results(), [oa, ob], [ta, tb])
    assert ga.position_results() == []  # pose fixes report through their own getter
    _close(pair, "orientation, full")
    pair.feed_imu()
    pair.frame()
    assert ga.pose_results() == []


# ---- 4 ----
def test_pose_fixes_at_one_timestamp_form_one_relinearized_chain(pair):
    ga, gb = pair.ga, pair.gb
    pair.feed_imu()
    (t,) = pair.times(0.5)
    s1, s2 = np.array([1.0, -0.5, 0.3]), np.array([-0.8, 0.6, 0.2])  # two rigid bodies a metre off the IMU
    q2 = M.quat_boxplus(QS, np.array([-0.4, 0.1, 0.2]))
    Rs = np.diag([1e-6] * 3 + [1e-5] * 3)  # 1 mrad, 3 mm: the first fix moves the state by most of the shift
    gb.propagate(t)
    x0 = gb.get_imu_state()[1]
    imu = _imu_id(gb)
    d = np.array([0.004, -0.003, 0.005, 0.03, -0.02, 0.025])
    # both measurements are fixed from the state before the first update
    z1 = (M.quat_boxplus(M.quat_multiply(QS, x0[0:4]), d[:3]), x0[4:7] + M.quat_2_Rot(x0[0:4]).T @ s1 + d[3:])
    z2 = (M.quat_boxplus(M.quat_multiply(q2, x0[0:4]), d[:3]), x0[4:7] + M.quat_2_Rot(x0[0:4]).T @ s2 + d[3:])
    res2_0, H2_0 = Q.pose_model(x0[0:4], x0[4:7], s2, q2, z2[0], z2[1], Q.FULL, False, False, np.float64)
    _, _, o1 = _explicit_pose(gb, t, Rs, z=z1, qS=QS, s=s1)
    x1, P1 = gb.get_imu_state()[1], gb.get_cov()
    res2_1, H2_1 = Q.pose_model(x1[0:4], x1[4:7], s2, q2, z2[0], z2[1], Q.FULL, False, False, np.float64)
    _, _, o2 = _explicit_pose(gb, t, Rs, z=z2, qS=q2, s=s2)
    assert o1["applied"] and o2["applied"]
    idx = np.arange(imu, imu + 6)
    dx_relin = M.ekf_update_R_ref(P1, idx, H2_1, res2_1, Rs, dtype=np.float64)[1]
    dx_prior = M.ekf_update_R_ref(P1, idx, H2_0, res2_0, Rs, dtype=np.float64)[1]
    scale = np.max(np.abs(gb.get_state_vector()[0]))
    gap = np.max(np.abs(dx_relin - dx_prior)) / scale
    print("POSERELIN dx gap / max|x| %.3e (device dx vs relinearized %.3e)" %
          (gap, np.max(np.abs(o2["dx"] - dx_relin)) / scale))
    assert gap > 1e-8, "the pair does not tell a relinearized chain from one linearized at the prior state"
    assert ga.feed_measurement_pose(t, z1[0], Rs, z_p=z1[1], q_ItoS=QS, p_SinI=s1)
    assert ga.feed_measurement_pose(t, z2[0], Rs, z_p=z2[1], q_ItoS=q2, p_SinI=s2)
    pair.frame()
    _same_results(ga.pose_results(), [o1, o2], [t, t])
    _close(pair, "same-time chain")


def test_nine_pose_fixes_at_one_timestamp_run_as_two_chains(pair):
    """a chain holds 8 fixes: the ninth is linearized from the host mean the first eight left"""
    ga, gb = pair.ga, pair.gb
    pair.feed_imu()
    (t,) = pair.times(0.5)
    fixes, outs = [], []
    for k in range(9):
        s = np.array([0.1 * k, -0.05, 0.02 * k])
        qS = M.quat_boxplus(QS, np.array([0.05 * k, 0.0, -0.03 * k]))
        full = k % 2 == 0
        d = 1e-3 * np.array([1.0, -1.5, 1.0, 2.0, 1.5, -1.0]) * (1.0 + 0.05 * k)  # half a sigma per component
        zq, zp, o = _explicit_pose(gb, t, R6 if full else R3Q, d=d if full else d[:3], qS=qS, s=s)
        fixes.append((zq, zp, qS, s))
        outs.append(o)
    assert all(o["applied"] for o in outs)
    for zq, zp, qS, s in fixes:
        assert ga.feed_measurement_pose(t, zq, R3Q if zp is None else R6, z_p=zp, q_ItoS=qS, p_SinI=s)
    pair.frame()
    _same_results(ga.pose_results(), outs, [t] * 9)
    _close(pair, "nine at one time")


# ---- 5 ----
def test_pose_position_and_uwb_at_one_timestamp_and_interleaved(euroc_yaml):
    import uvio_amd as U
    opts, anchors, sim, (ga, gb) = _uwb_setup(euroc_yaml, lambda op: (U.VioManager(op), U.VioManager(op)))
    last = {}
    sim.run([ga, gb], n_frames=10, on_frame=lambda nf, t: last.update(t=t),
            after_init=lambda m: m.try_to_initialize_uwb_anchors(anchors))
    p = Pair(opts, sim, ga, gb, last["t"])
    assert p.identical(), "two handles on one stream differ: nothing below can be compared"
    p.feed_imu()
    t1, tf, t2, t3 = p.times(0.25, 0.4, 0.55, 0.75)
    r1 = _true_range(sim, opts, anchors[3], t1) + 0.03
    r2 = _true_range(sim, opts, anchors[0], t2) + 0.03
    # B at t1: the UWB message goes first at one timestamp, then the fixes in A's feed order
    gb.propagate(t1)
    assert gb.uwb_update_single(t1, anchors[3].id, r1), "a consistent range was gated"
    zq1, zp1, o1 = _explicit_pose(gb, t1, R6, d=[2e-3, -1e-3, 3e-3, 0.004, 0.003, -0.005])
    zf1, of1 = _explicit_fix(gb, t1, [0.01, -0.004, 0.006], ARM, R3)
    zq1b, _, o1b = _explicit_pose(gb, t1, R3Q, d=[-2e-3, 1e-3, 1e-3])
    # interleaved times: a position fix, then a range, then a pose
    zf2, of2 = _explicit_fix(gb, tf, [0.003, 0.002, -0.004], ARM, R3)
    gb.propagate(t2)
    assert gb.uwb_update_single(t2, anchors[0].id, r2), "a consistent range was gated"
    zq3, zp3, o3 = _explicit_pose(gb, t3, R6, d=[1e-3, 2e-3, -2e-3, -0.003, 0.004, 0.002])
    assert all(o["applied"] for o in (o1, of1, o1b, of2, o3))
    # A: fed out of time order on purpose; at t1 the fixes keep their feed order: pose, position, pose
    assert ga.feed_measurement_pose(t3, zq3, R6, z_p=zp3, q_ItoS=QS, p_SinI=ARM)
    assert ga.feed_measurement_pose(t1, zq1, R6, z_p=zp1, q_ItoS=QS, p_SinI=ARM)
    ga.feed_measurement_uwb(t2, [anchors[0].id], [r2])
    assert ga.feed_measurement_position(t1, zf1, R3, p_SinI=ARM)
    assert ga.feed_measurement_position(tf, zf2, R3, p_SinI=ARM)
    assert ga.feed_measurement_pose(t1, zq1b, R3Q, q_ItoS=QS)
    ga.feed_measurement_uwb(t1, [anchors[3].id], [r1])
    p.frame()
    _same_results(ga.pose_results(), [o1, o1b, o3], [t1, t1, t3])
    _same_results(ga.position_results(), [of1, of2], [t1, tf])
    _close(p, "uwb + pose + position + pose | position | uwb | pose")
    ga.close()
    gb.close()


# ---- 6 ----
def test_aux_mounting_rotation_over_three_frames(pair_fixed_intrinsics):
    from uvio_amd.sim import rot_2_quat
    pair = pair_fixed_intrinsics
    ga, gb, sim = pair.ga, pair.gb, pair.sim
    turn = np.deg2rad(5.0) * np.array([0.6, -0.64, 0.48])  # a unit axis: the sensor is turned 5 degrees
    q_true = M.quat_boxplus(QS, 2.0 * np.tan(np.linalg.norm(turn) / 2) * turn / np.linalg.norm(turn))
    arm_true = np.array([0.25, -0.10, 0.15])
    arm0 = arm_true + np.array([0.05, -0.04, 0.03])
    PRIORQ = np.array([[2e-2, 1e-3, -2e-3], [1e-3, 3e-2, 5e-4], [-2e-3, 5e-4, 1e-2]])  # ~8 degrees

    def angle(q):
        dq = M.quat_multiply(q_true, Q.quat_inv(q))
        return 2.0 * np.arcsin(min(1.0, np.linalg.norm(dq[:3])))

    assert abs(angle(QS) - np.deg2rad(5.0)) < 1e-12
    for _ in range(2):  # to a full clone window: from here on every frame marginalizes the oldest clone
        pair.feed_imu()
        pair.frame()
    assert pair.identical()
    arm_a, arm_b = ga.add_state(arm0, PRIOR3), gb.add_state(arm0, PRIOR3)
    rot_a, rot_b = ga.add_quat_state(QS, PRIORQ), gb.add_quat_state(QS, PRIORQ)
    assert (arm_a, rot_a) == (arm_b, rot_b) and pair.identical() and ga.aux_count() == (2, 6)
    rid0 = ga.aux_state(rot_a)[0]
    m0 = ga.get_marginal_cov([(rid0, 3)])
    assert np.array_equal(m0, PRIORQ)
    offsets = []
    for step in range(3):
        pair.feed_imu()
        (t,) = pair.times(0.4 + 0.1 * step)
        offsets.append((ga.aux_state(arm_a)[0], ga.aux_state(rot_a)[0]))
        R_GtoI = sim.traj.R_ItoG(t).T
        q_GtoI = rot_2_quat(R_GtoI)
        assert np.max(np.abs(M.quat_2_Rot(q_GtoI) - R_GtoI)) < 1e-12
        z = (M.quat_multiply(q_true, q_GtoI), sim.traj.pos(t) + sim.traj.R_ItoG(t) @ arm_true)
        _, _, ob = _explicit_pose(gb, t, R6, z=z, rot_h=rot_b, arm_h=arm_b, chi2_mult=INF)
        assert ob["applied"]
        assert ga.feed_measurement_pose(t, z[0], R6, z_p=z[1], rot_handle=rot_a, arm_handle=arm_a, chi2_mult=INF)
        pair.frame()
        _same_results(ga.pose_results(), [ob], [t])
        _close(pair, "aux rotation %d" % step)
        assert ga.aux_state(rot_a)[0] == gb.aux_state(rot_b)[0]
    rid, qv = ga.aux_state(rot_a)
    arm = ga.aux_state(arm_a)[1]
    m1 = ga.get_marginal_cov([(rid, 3)])
    print("POSEROT offsets %s angle %.4f -> %.4f deg, arm error %.4f -> %.4f, marginal trace %.3e -> %.3e" %
          (offsets, np.rad2deg(angle(QS)), np.rad2deg(angle(qv)), np.linalg.norm(arm0 - arm_true),
           np.linalg.norm(arm - arm_true), np.trace(m0), np.trace(m1)))
    assert len(set(offsets)) > 1, "no clone was marginalized in front of the variables"
    assert qv.size == 4 and abs(np.linalg.norm(qv) - 1.0) < 1e-14
    assert angle(qv) < 0.5 * angle(QS)
    assert np.all(np.linalg.eigvalsh(m0 - m1) > 0), "the rotation's marginal did not shrink"
    assert np.linalg.norm(arm - arm_true) < np.linalg.norm(arm0 - arm_true)
    for m, hs in ((ga, (arm_a, rot_a)), (gb, (arm_b, rot_b))):
        for h in hs:
            m.remove_state(h)
    assert ga.aux_count() == (0, 0)


def test_pose_drops_refusals_gate_and_feed_time_errors(pair):
    import uvio_amd as U
    from uvio_amd import _native as N
    from uvio_amd.sim import rot_2_quat
    ga, gb, sim = pair.ga, pair.gb, pair.sim

    def truth(t):
        return (M.quat_multiply(QS, rot_2_quat(sim.traj.R_ItoG(t).T)), sim.traj.pos(t) + sim.traj.R_ItoG(t) @ ARM)

    # a dead rotation handle: refused; a pose 1 rad off: gated; one at the frame time: dropped.  B only propagates
    pair.feed_imu()
    ta, tb, t_frame = pair.times(0.4, 0.6, 1.0)
    ha, hb = ga.add_quat_state(QS, PRIOR3), gb.add_quat_state(QS, PRIOR3)
    va, vb = ga.add_state(ARM, PRIOR3), gb.add_state(ARM, PRIOR3)
    za, zb = truth(ta), truth(tb)
    assert ga.feed_measurement_pose(ta, za[0], R6, z_p=za[1], rot_handle=ha, arm_handle=va)
    assert ga.feed_measurement_pose(tb, M.quat_boxplus(zb[0], [1.0, 0.0, 0.0]), R3Q, q_ItoS=QS)
    assert ga.feed_measurement_pose(t_frame, za[0], R3Q, q_ItoS=QS)
    with pytest.raises(RuntimeError, match="E_ARG"):  # the kinds are told apart though both have 3 dimensions
        ga.feed_measurement_pose(ta, za[0], R6, z_p=za[1], rot_handle=va, arm_handle=va)
    with pytest.raises(RuntimeError, match="E_ARG"):
        ga.feed_measurement_pose(ta, za[0], R6, z_p=za[1], rot_handle=ha, arm_handle=ha)
    with pytest.raises(RuntimeError, match="E_ARG"):
        ga.feed_measurement_position(ta, za[1], R3, aux_handle=ha)
    for m, hs in ((ga, (ha, va)), (gb, (hb, vb))):
        for h in hs:
            m.remove_state(h)
    for t in (ta, tb):
        gb.propagate(t)
    pair.frame()
    res = ga.pose_results()
    assert [(r["t"], r["status"]) for r in res] == [(ta, 3), (tb, 1), (t_frame, 2)], res
    assert res[1]["chi2"] > U.chi2_95(3)
    assert pair.identical()

    # feed-time refusals leave the queue and the state untouched
    pair.feed_imu()
    (t,) = pair.times(0.5)
    x0, P0 = ga.get_state_vector()[0], ga.get_cov()
    zq, zp = truth(t)
    bad = [dict(z_q=3.0 * zq), dict(z_q=0.4 * zq), dict(z_q=[np.nan, 0.0, 0.0, 1.0]), dict(q_ItoS=2.5 * QS),
           dict(z_p=[0.0, np.inf, 0.0]), dict(t=float("nan")), dict(R=np.triu(np.full((6, 6), np.inf))),
           dict(R=np.diag([1.0, 1.0, 1.0, 0.0, 1.0, 1.0])), dict(R=np.diag([1.0, -1.0, 1.0, 1.0, 1.0, 1.0])),
           dict(p_SinI=[0.0, np.nan, 0.0]), dict(chi2_mult=0.0), dict(chi2_mult=float("nan")),
           dict(rot_handle=ha), dict(arm_handle=12345)]
    for over in bad:
        kw = dict(t=t, z_q=zq, R=R6, z_p=zp, q_ItoS=QS, p_SinI=ARM)
        kw.update(over)
        with pytest.raises(RuntimeError, match="E_ARG"):
            ga.feed_measurement_pose(kw.pop("t"), kw.pop("z_q"), kw.pop("R"), **kw)
    lib, dp = N.load(), C.POINTER(C.c_double)
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (zq, zp, R6, QS, ARM)]
    pq, pp, pR, pS, pA = [a.ctypes.data_as(dp) for a in arrs]
    qd = C.c_int(-3)
    feed = lib.uvio_hp_feed_pose
    assert feed(ga._h, t, 0, pq, pp, pR, 6, pS, 0, pA, 0, 1.0, C.byref(qd)) == N.E_ARG  # a bad mode
    assert feed(ga._h, t, 3, pq, pp, pR, 6, pS, 0, pA, 0, 1.0, C.byref(qd)) == N.E_ARG
    assert feed(ga._h, t, N.POSE_FULL, pq, None, pR, 6, pS, 0, pA, 0, 1.0, C.byref(qd)) == N.E_ARG  # no z_p in FULL mode
    assert feed(ga._h, t, N.POSE_FULL, pq, pp, pR, 5, pS, 0, pA, 0, 1.0, C.byref(qd)) == N.E_ARG  # ldr < r
    assert feed(ga._h, t, N.POSE_ORIENTATION, pq, None, pR, 2, pS, 0, None, 0, 1.0, C.byref(qd)) == N.E_ARG
    assert feed(ga._h, t, N.POSE_ORIENTATION, pq, None, pR, 6, None, 0, None, 0, 1.0, C.byref(qd)) == N.E_ARG  # no q_ItoS
    # the queue holds 256 fixes across both kinds; these sit at the frame time, where the frame drops them
    (t_frame,) = pair.times(1.0)
    for k in range(128):
        assert ga.feed_measurement_pose(t_frame, zq, R3Q, q_ItoS=QS)
        assert ga.feed_measurement_position(t_frame, zp, R3, p_SinI=ARM)
    with pytest.raises(RuntimeError, match="E_CAPACITY"):
        ga.feed_measurement_pose(t, zq, R3Q, q_ItoS=QS)
    with pytest.raises(RuntimeError, match="E_CAPACITY"):
        ga.feed_measurement_position(t, zp, R3, p_SinI=ARM)
    assert np.array_equal(ga.get_state_vector()[0], x0) and np.array_equal(ga.get_cov(), P0)
    pair.frame()
    res = ga.pose_results()
    assert len(res) == 128 and all(r["status"] == 2 and r["t"] == t_frame for r in res)
    assert len(ga.position_results()) == 128
    n = C.c_int(0)
    assert lib.uvio_hp_get_pose_results(ga._h, None, None, None, 127, C.byref(n)) == N.E_CAPACITY and n.value == 128
    assert pair.identical()
    # the queue is empty again: a pose is taken and applied
    pair.feed_imu()
    (t,) = pair.times(0.5)
    zq, zp, ob = _explicit_pose(gb, t, R6, d=[1e-3, -2e-3, 1e-3, 0.004, 0.0, -0.003])
    assert ga.feed_measurement_pose(t, zq, R6, z_p=zp, q_ItoS=QS, p_SinI=ARM)
    pair.frame()
    _same_results(ga.pose_results(), [ob], [t])


# ---- 7 ----
def _without_var(x, meta, P, aid):
    """state vector, meta and covariance with the variable at covariance offset aid removed"""
    k, xs, ms = 0, [], []
    dim = int([size for _, vid, size in meta if vid == aid][0])
    keep = np.ones(P.shape[0], bool)
    keep[aid:aid + dim] = False
    for kind, vid, size in meta:
        vlen = size + 1 if kind in (0, 2, 3, 7) else size
        if vid != aid:
            xs.append(x[k:k + vlen])
            ms.append((kind, vid - dim if vid > aid else vid, size))
        k += vlen
    return np.concatenate(xs), np.array(ms, dtype=np.int32), P[np.ix_(keep, keep)]


def test_quaternion_variable_append_boxplus_meta_walk_remove(pair):
    g = pair.ga
    pair.feed_imu()
    x0, m0 = g.get_state_vector()
    P0 = g.get_cov()
    N0 = P0.shape[0]
    with pytest.raises(RuntimeError, match="E_ARG"):
        g.add_quat_state(3.0 * QS, PRIOR3)
    with pytest.raises(RuntimeError, match="E_ARG"):
        g.add_quat_state(0.4 * QS, PRIOR3)
    with pytest.raises(RuntimeError, match="E_ARG"):
        g.add_quat_state([np.nan, 0.0, 0.0, 1.0], PRIOR3)
    with pytest.raises(RuntimeError, match="E_ARG"):
        g.add_quat_state(QS, np.diag([1.0, 0.0, 1.0]))
    assert g.aux_count() == (0, 0) and np.array_equal(g.get_cov(), P0)
    sigma = np.array([2e-3, 0.0, 5e-3])
    prior = PRIOR3.copy()
    prior[np.tril_indices(3, -1)] = np.nan  # the strictly lower triangle is never read
    h = g.add_quat_state(1.7 * QS, prior, walk_sigma=sigma)  # normalized on entry
    assert g.aux_count() == (1, 3)
    aid, qv = g.aux_state(h)
    assert aid == N0 and qv.size == 4 and np.max(np.abs(qv - QS)) < 4e-16 and abs(np.linalg.norm(qv) - 1.0) < 4e-16
    x1, m1 = g.get_state_vector()
    P1 = g.get_cov()
    # the appended rows and columns against the float64 replay, bit for bit
    assert np.array_equal(P1, A.append_ref(P0, np.triu(PRIOR3)))
    assert [tuple(m) for m in m1 if m[0] == 7] == [(7, N0, 3)] and np.array_equal(m1[:-1], m0)
    assert x1.size == x0.size + 4 and np.array_equal(x1[:-4], x0) and np.array_equal(x1[-4:], qv)
    assert np.array_equal(g.get_fej_vector()[-4:], qv)  # value and first estimate are set together
    # measurement_update on its columns: boxplus, checked against NumPy
    out = g.measurement_update([(aid, 3)], np.eye(3), [0.03, -0.02, 0.05], 1e-4 * np.eye(3))
    assert out["applied"]
    dth = out["dx"][aid:aid + 3]
    assert np.max(np.abs(dth)) > 1e-3
    q2 = g.aux_state(h)[1]
    assert np.max(np.abs(q2 - M.quat_boxplus(qv, dth))) < 4e-16 and abs(np.linalg.norm(q2) - 1.0) < 4e-16
    assert np.array_equal(g.get_state_vector()[0][-4:], q2)
    # the walk: uvio_hp_propagate advances the state time by dt, the diagonal grows by fl(sigma^2 dt)
    P2 = g.get_cov()
    t0 = g.get_imu_state()[0]
    (t,) = pair.times(0.5)
    g.propagate(t)
    dt = np.float64(g.get_imu_state()[0]) - np.float64(t0)
    P3 = g.get_cov()
    assert np.array_equal(P3[aid:aid + 3, aid:aid + 3].diagonal(), P2[aid:aid + 3, aid:aid + 3].diagonal() + sigma * sigma * dt)
    assert P3[aid, aid + 1] == P2[aid, aid + 1] and P3[aid + 1, aid + 2] == P2[aid + 1, aid + 2]
    assert np.array_equal(g.aux_state(h)[1], q2)
    # remove: marginalized, the rest is what it was
    xb, mb = g.get_state_vector()
    xr, mr, Pr = _without_var(xb, mb, P3, aid)
    g.remove_state(h)
    assert g.aux_count() == (0, 0)
    xa, ma = g.get_state_vector()
    assert np.array_equal(ma, mr) and np.array_equal(xa, xr) and np.array_equal(g.get_cov(), Pr)
    with pytest.raises(RuntimeError, match="E_ARG"):
        g.aux_state(h)


def test_idle_quaternion_passenger_changes_nothing(euroc_yaml):
    import uvio_amd as U
    from uvio_amd.sim import SimStream
    ov = dict(OVERRIDES, max_clone_size=5)  # the window fills, and clones leave, within the ten frames
    opts, opts8 = U.load_options(euroc_yaml, **ov), U.load_options(euroc_yaml, max_aux_dim=8, **ov)
    sim = SimStream(opts, duration=14 / opts.track_frequency + 1.2, seed=7, spawn=60, frac_long=0.3)
    plain, passenger = U.VioManager(opts), U.VioManager(opts8)
    st = {"h": None, "ids": [], "identical": True, "checked": 0}

    def on_frame(nf, t):
        if nf == 3:  # three clones are in front of the variable
            st["h"] = passenger.add_quat_state(QS, PRIOR3)
        if st["h"] is None:
            return
        xp, mp = plain.get_state_vector()
        Pp = plain.get_cov()
        aid, val = passenger.aux_state(st["h"])
        st["ids"].append(aid)
        x, meta = passenger.get_state_vector()
        P = passenger.get_cov()
        assert [tuple(m) for m in meta if m[0] == 7] == [(7, aid, 3)]
        assert np.array_equal(val, QS)
        assert np.array_equal(P[aid:aid + 3, aid:aid + 3], PRIOR3), nf
        rest = np.ones(P.shape[0], bool)
        rest[aid:aid + 3] = False
        assert np.all(P[aid:aid + 3][:, rest] == 0.0) and np.all(P[rest][:, aid:aid + 3] == 0.0), nf
        x1, m1, P1 = _without_var(x, meta, P, aid)
        assert np.array_equal(m1, mp)
        st["identical"] = st["identical"] and np.array_equal(x1, xp) and np.array_equal(P1, Pp)
        st["checked"] += 1

    sim.run([plain, passenger], n_frames=10, on_frame=on_frame)
    print("POSEIDLE checked %d frames, offsets %s, bit-identical %s" % (st["checked"], st["ids"], st["identical"]))
    assert st["checked"] == 8 and st["identical"]
    assert len(set(st["ids"])) > 1 and st["ids"][-1] < st["ids"][0], "the offset never moved: no clone left in front"
    for m in (plain, passenger):
        m.close()


# ---- 8 ----
def test_cpp_facade_pose_on_the_device(tmp_path):
    from test_facade_pose import CFG, build_check, run_env
    exe = build_check(tmp_path)
    r = subprocess.run([exe, CFG, "gpu"], capture_output=True, text=True, timeout=120, env=run_env())
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "refused: code -1" in r.stdout and "POSE ok" in r.stdout
