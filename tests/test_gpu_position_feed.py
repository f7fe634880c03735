"""Buffered position fixes on the device: uvio_hp_feed_position / uvio_hp_get_position_results on a handle and the
chain's three kernels (k_fix_rows -> k_chain_M -> k_chain_update) on a standalone covariance
(uvio_hp_debug_position_update_p).

1. Numerics of the three kernels against the extended-precision reference (tests/fix_ref.py): N = 15, 16, 17, 33 (the
   edges of the 16-row tiles), ld = N and N + 5 (the padding comes back untouched), r = 1, 2, 3, the lever arm a
   constant, a state variable directly behind the IMU pose and one at N - 3, R dense and graded.  P+ exactly symmetric,
   and in ekf_ref.scaled_err / scaled_dx_err units
       e_dev <= RATIO * max(e_f64, 16 * 2^-52)
   with e_f64 the float64 NumPy comparator's error against the same reference.  RATIO = 4 x the worst measured ratio,
   rounded up to a power of two (the procedure of tests/test_gpu_meas_update.py).  Measured on MI355X over the 72 cases:
       dx   1.24  N16-r1-const  (device 1.89e-14, float64 1.53e-14)
       P+   0.50  N16-r3-const  (device 5.57e-15, float64 1.11e-14)
   so RATIO = 8.  The device forms H and the residual in another operation order than NumPy and sums S and W W^T with
   explicit FMAs, so a small constant over the comparator is expected.
   chi2 within 1e-10 (relative) of the reference's (measured: 8.0e-14 at worst), the gate applied on both sides of it.
2. Buffered equals explicit: handle A queues two fixes (r = 3 on a constant lever arm, r = 1) inside one frame interval,
   handle B does propagate + measurement_update at the same times; after the frame state time and per-fix status are
   equal, chi2 within 1e-10, x and P within tests/test_gpu_parity.py's 1e-10 (max abs diff / max abs value).
3. Interleaved with UWB: a range at t1, a fix at t2, a range at t3 inside one frame interval, buffered on A, explicit
   on B.
4. An aux lever arm through the buffered path over three frames while clones are marginalized in front of it, against
   position_fix_lever_arm on B; the arm moves towards the simulated one.  (With fixed camera intrinsics: see
   pair_fixed_intrinsics for what online intrinsic calibration does to this comparison from the 11th frame on.)
5. Two fixes at one timestamp: one chain, the second linearized at the state the first left.  Nine at one timestamp: two
   chains.
6. Drops, refusals, the gate, and the feed-time errors.
7. The C++ facade on the device (tests/cpp/facade_fix_check.cpp).
All inputs are consistent fixes or plainly malformed arguments.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ekf_ref as E  # noqa: E402
import fix_ref as F  # noqa: E402
import meas_ref as M  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not E.HAVE_EXTENDED, reason=E.REASON)]

from test_gpu_meas_update import _feed_imu_until, _frame_index, _rel, _true_range, _uwb_setup  # noqa: E402

RATIO = 8.0
FLOOR = 16 * 2.0 ** -52
PAD = -7.25  # uvio_amd.manager._padded's filler
INF = float("inf")
OVERRIDES = dict(max_msckf_in_update=60, max_slam_features=10, max_slam_in_update=5, dt_slam_delay=0.3)
PRIOR3 = np.array([[4e-2, 1e-3, -2e-3], [1e-3, 9e-2, 5e-4], [-2e-3, 5e-4, 1e-2]])
R3 = 9e-4 * np.array([[1.0, 0.2, -0.1], [0.2, 1.5, 0.3], [-0.1, 0.3, 0.8]])  # a 3 cm sensor with correlated axes
EZ = np.array([[0.0, 0.0, 1.0]])


# ---- 1 ----
@pytest.mark.parametrize("N", [15, 16, 17, 33])
def test_three_kernels_against_extended_reference(N):
    import uvio_amd as U
    worst = {"P": 0.0, "dx": 0.0}
    for r in (1, 2, 3):
        for aux_id in (-1, 6, N - 3):
            k = F.fix_case(N, r, aux_id, seed=9000 + 100 * N + 10 * r + (aux_id > 0) + (aux_id > 6))
            args = (k.imu_id, k.q, k.p, k.s, k.C, k.z, k.R, k.aux_id)
            Pr, dxr, c_ref = F.fix_update_ref(k.P, *args)
            P6, dx6, _ = F.fix_update_ref(k.P, *args, dtype=np.float64)
            c_ref = float(c_ref)
            e_64, x_64 = E.scaled_err(P6, Pr, k.P), E.scaled_dx_err(dx6, dxr, k.P)
            for ld in (N, N + 5):
                tag = "N%d-ld%d-r%d-aux%d" % (N, ld, r, aux_id)
                buf, dxg, chi2, applied = U.position_update_p(k.P, *args[:7], aux_id=aux_id, ld=ld)
                Pg = buf[:, :N]
                e_dev, x_dev = E.scaled_err(Pg, Pr, k.P), E.scaled_dx_err(dxg, dxr, k.P)
                rp, rx = e_dev / max(e_64, FLOOR), x_dev / max(x_64, FLOOR)
                worst["P"], worst["dx"] = max(worst["P"], rp), max(worst["dx"], rx)
                print("FIXPATH %s P dev %.3e f64 %.3e ratio %.2f dx dev %.3e f64 %.3e ratio %.2f chi2 rel %.2e" %
                      (tag, e_dev, e_64, rp, x_dev, x_64, rx, abs(chi2 - c_ref) / c_ref))
                assert applied and np.all(buf[:, N:] == PAD), tag
                assert np.array_equal(Pg, Pg.T), tag
                assert e_dev <= RATIO * max(e_64, FLOOR), (tag, e_dev, e_64)
                assert x_dev <= RATIO * max(x_64, FLOOR), (tag, x_dev, x_64)
                assert abs(chi2 - c_ref) < 1e-10 * c_ref, (tag, chi2, c_ref)
                # the gate on both sides of the reference's chi2 (test_gate_compares_the_reference_chi2)
                b1, d1, c1, a1 = U.position_update_p(k.P, *args[:7], aux_id=aux_id, ld=ld, chi2_thr=c_ref * (1 + 1e-6))
                assert a1 and c1 == chi2 and np.array_equal(b1, buf) and np.array_equal(d1, dxg), tag
                b0, d0, c0, a0 = U.position_update_p(k.P, *args[:7], aux_id=aux_id, ld=ld, chi2_thr=c_ref * (1 - 1e-6))
                assert not a0 and c0 == chi2 and np.all(d0 == 0.0), tag
                assert np.array_equal(b0[:, :N], k.P) and np.all(b0[:, N:] == PAD), tag
    print("FIXWORST N%d P ratio %.2f dx ratio %.2f" % (N, worst["P"], worst["dx"]))


def test_standalone_refuses_an_indefinite_S():
    """R's diagonal is positive but R is far from positive definite: the factor's pivot check refuses, P is untouched"""
    import uvio_amd as U
    k = F.fix_case(17, 2, -1, seed=41)
    pred, H = F.fix_model(k.q, k.p, k.s, k.C, False, np.float64)
    big = 1e3 * np.max(np.abs(H @ k.P[:6, :6] @ H.T))
    with pytest.raises(RuntimeError, match="E_ARG"):
        U.position_update_p(k.P, 0, k.q, k.p, k.s, k.C, k.z, big * np.array([[1.0, 10.0], [10.0, 1.0]]))
    buf, dx, chi2, applied = U.position_update_p(k.P, 0, k.q, k.p, k.s, k.C, k.z, k.R)
    assert applied and not np.array_equal(buf, k.P)


# ---- two handles on one stream ----
class Pair:
    def __init__(self, opts, sim, ga, gb, last_t):
        self.opts, self.sim, self.ga, self.gb = opts, sim, ga, gb
        self.i = _frame_index(sim, last_t)

    def times(self, *fracs):
        t0, t1 = float(self.sim.cam_t[self.i]), float(self.sim.cam_t[self.i + 1])
        return [t0 + f * (t1 - t0) for f in fracs]

    def feed_imu(self):
        _feed_imu_until(self.sim, [self.ga, self.gb], self.sim.cam_t[self.i], self.sim.cam_t[self.i + 1])

    def frame(self):
        self.i += 1
        for m in (self.ga, self.gb):
            m.feed_measurement_simulation(float(self.sim.cam_t[self.i]), list(range(self.sim.K)), self.sim.frames[self.i])

    def identical(self):
        return (self.ga.get_imu_state()[0] == self.gb.get_imu_state()[0] and
                np.array_equal(self.ga.get_state_vector()[0], self.gb.get_state_vector()[0]) and
                np.array_equal(self.ga.get_state_vector()[1], self.gb.get_state_vector()[1]) and
                np.array_equal(self.ga.get_cov(), self.gb.get_cov()))

    def close_enough(self, tag):
        """tests/test_gpu_parity.py's lock-step measures and bound"""
        xa, ma = self.ga.get_state_vector()
        xb, mb = self.gb.get_state_vector()
        assert self.ga.get_imu_state()[0] == self.gb.get_imu_state()[0]
        assert np.array_equal(ma, mb), "state layouts differ"
        ex, eP = _rel(xa, xb), _rel(self.ga.get_cov(), self.gb.get_cov())
        print("FIXPAIR %s x rel %.2e P rel %.2e" % (tag, ex, eP))
        assert ex < 1e-10 and eP < 1e-10, (tag, ex, eP)


def _imu_id(g):
    return int([m for m in g.get_state_vector()[1] if m[0] == 0][0][1])


def _explicit_fix(g, t, offset, s, R, Cm=None, chi2_mult=1.0):
    """propagate to t (unless already there), then the fix z = prediction + offset through measurement_update;
    returns (z, result)"""
    import uvio_amd as U
    from uvio_amd.manager import position_fix_jacobian
    if g.get_imu_state()[0] < t:
        g.propagate(t)
    x = g.get_imu_state()[1]
    pred, H = position_fix_jacobian(x[0:4], x[4:7], s)
    Cm = np.eye(3) if Cm is None else np.asarray(Cm, dtype=np.float64)
    z = Cm @ pred + np.asarray(offset, dtype=np.float64)
    out = g.measurement_update([(_imu_id(g), 6)], Cm @ H, z - Cm @ pred, R, chi2_mult * U.chi2_95(Cm.shape[0]))
    return z, out


def _same_results(res, outs, times):
    assert [r["status"] for r in res] == [0 if o["applied"] else 1 for o in outs], (res, outs)
    assert [r["t"] for r in res] == list(times)
    for r, o in zip(res, outs):
        print("FIXCHI2 t %.6f buffered %.17g explicit %.17g" % (r["t"], r["chi2"], o["chi2"]))
        assert abs(r["chi2"] - o["chi2"]) < 1e-10 * o["chi2"]


@pytest.fixture(scope="module")
def stream(euroc_yaml):
    """the options and the simulated stream every pair runs on (read-only)"""
    import uvio_amd as U
    from uvio_amd.sim import SimStream
    opts = U.load_options(euroc_yaml, max_aux_dim=8, **OVERRIDES)
    return opts, SimStream(opts, duration=(10 + 8) / opts.track_frequency + 1.2, seed=7, spawn=60, frac_long=0.3)


def _pair(opts, sim):
    import uvio_amd as U
    ga, gb = U.VioManager(opts), U.VioManager(opts)
    last = {}
    sim.run([ga, gb], n_frames=10, on_frame=lambda nf, t: last.update(t=t))
    p = Pair(opts, sim, ga, gb, last["t"])
    assert p.identical(), "two handles on one stream differ: nothing below can be compared"
    return p


@pytest.fixture
def pair(stream):
    """a fresh pair of handles after 10 simulated frames: every test starts from two handles that agree to the bit"""
    p = _pair(*stream)
    yield p
    p.ga.close()
    p.gb.close()


@pytest.fixture
def pair_fixed_intrinsics(stream, euroc_yaml):
    """The pair for comparisons on frames that marginalize a clone (from the 11th on).  A frame undistorts its
    observations with the intrinsics of the moment they are fed.  The explicit path's fix lies before that feed, the
    buffered one behind the tracking (where the reference puts its UWB updates), so with the intrinsics calibrated
    online the newest observations' normalized coordinates differ by what the fix moved the intrinsics (measured:
    1e-7 of the state after one such frame's update; frame 10 uses none of its own observations and agrees to 1e-16
    either way).  That is the order of two operations, not arithmetic: with fixed intrinsics the paths agree again."""
    import uvio_amd as U
    p = _pair(U.load_options(euroc_yaml, max_aux_dim=8, do_calib_camera_intrinsics=0, **OVERRIDES), stream[1])
    yield p
    p.ga.close()
    p.gb.close()


# ---- 2 ----
def test_buffered_fixes_equal_the_explicit_path(pair):
    ga, gb = pair.ga, pair.gb
    assert ga.position_results() == []
    pair.feed_imu()
    ta, tb = pair.times(0.3, 0.65)
    s = np.array([0.2, -0.05, 0.1])
    R1 = np.array([[4e-4]])
    za, oa = _explicit_fix(gb, ta, [0.01, -0.004, 0.006], s, R3)
    zb, ob = _explicit_fix(gb, tb, [0.008], np.zeros(3), R1, Cm=EZ)
    assert oa["applied"] and ob["applied"], "a consistent fix was gated"
    assert ga.feed_measurement_position(ta, za, R3, p_SinI=s)
    assert ga.feed_measurement_position(tb, zb, R1, Cm=EZ)
    assert not pair.identical()
    pair.frame()
    _same_results(ga.position_results(), [oa, ob], [ta, tb])
    pair.close_enough("two fixes")
    # the results are the last feed's: a frame without fixes reports none
    pair.feed_imu()
    pair.frame()
    assert ga.position_results() == []


# ---- 5 ----
def test_fixes_at_one_timestamp_form_one_relinearized_chain(pair):
    from uvio_amd.manager import position_fix_jacobian
    ga, gb = pair.ga, pair.gb
    pair.feed_imu()
    (t,) = pair.times(0.5)
    s1, s2 = np.array([1.0, -0.5, 0.3]), np.array([-0.8, 0.6, 0.2])  # two antennas a metre off the IMU
    Rs = 1e-5 * np.eye(3)  # a 3 mm sensor: the first fix moves the state by most of the shift
    gb.propagate(t)
    x0 = gb.get_imu_state()[1]
    imu = _imu_id(gb)
    # both measurements are fixed from the state before the first update: z_k = h_k(x0) + offset
    pred1, _ = position_fix_jacobian(x0[0:4], x0[4:7], s1)
    pred2, H2_0 = position_fix_jacobian(x0[0:4], x0[4:7], s2)
    shift = np.array([0.03, -0.02, 0.025])  # the body a few centimetres off the estimate: consistent with both antennas
    z1, z2 = pred1 + shift, pred2 + shift
    o1 = gb.position_fix(z1, s1, Rs)
    x1, P1 = gb.get_imu_state()[1], gb.get_cov()
    pred2_1, H2_1 = position_fix_jacobian(x1[0:4], x1[4:7], s2)
    o2 = gb.position_fix(z2, s2, Rs)
    assert o1["applied"] and o2["applied"]
    # what a chain that linearized both fixes at the prior state would have applied for the second one
    idx = np.arange(imu, imu + 6)
    dx_relin = M.ekf_update_R_ref(P1, idx, H2_1, z2 - pred2_1, Rs, dtype=np.float64)[1]
    dx_prior = M.ekf_update_R_ref(P1, idx, H2_0, z2 - pred2, Rs, dtype=np.float64)[1]
    scale = np.max(np.abs(gb.get_state_vector()[0]))
    gap = np.max(np.abs(np.asarray(dx_relin - dx_prior, dtype=np.float64))) / scale
    print("FIXRELIN dx gap / max|x| %.3e (device dx vs relinearized %.3e)" %
          (gap, np.max(np.abs(o2["dx"] - np.asarray(dx_relin, dtype=np.float64))) / scale))
    assert gap > 1e-8, "the pair does not tell a relinearized chain from one linearized at the prior state"
    for z, s in ((z1, s1), (z2, s2)):
        assert ga.feed_measurement_position(t, z, Rs, p_SinI=s)
    pair.frame()
    _same_results(ga.position_results(), [o1, o2], [t, t])
    pair.close_enough("same-time chain")


def test_nine_fixes_at_one_timestamp_run_as_two_chains(pair):
    """a chain holds 8 fixes: the ninth is linearized from the host mean the first eight left"""
    ga, gb = pair.ga, pair.gb
    pair.feed_imu()
    (t,) = pair.times(0.5)
    R1 = np.array([[4e-4]])
    fixes, outs = [], []
    for k in range(9):
        Cm, s = np.eye(3)[k % 3][None, :], np.array([0.1 * k, -0.05, 0.02 * k])
        z, o = _explicit_fix(gb, t, [0.002 * (k + 1)], s, R1, Cm=Cm)
        fixes.append((z, Cm, s))
        outs.append(o)
    assert all(o["applied"] for o in outs)
    for z, Cm, s in fixes:
        assert ga.feed_measurement_position(t, z, R1, Cm=Cm, p_SinI=s)
    pair.frame()
    _same_results(ga.position_results(), outs, [t] * 9)
    pair.close_enough("nine at one time")


# ---- 4 ----
def test_aux_lever_arm_over_three_frames(pair_fixed_intrinsics):
    pair = pair_fixed_intrinsics
    ga, gb, sim = pair.ga, pair.gb, pair.sim
    arm_true = np.array([0.25, -0.10, 0.15])
    arm0 = arm_true + np.array([0.05, -0.04, 0.03])
    for _ in range(2):  # to a full clone window: from here on every frame marginalizes the oldest clone
        pair.feed_imu()
        pair.frame()
    assert pair.identical()
    ha, hb = ga.add_state(arm0, PRIOR3), gb.add_state(arm0, PRIOR3)
    assert ha == hb and pair.identical()
    offsets = []
    for step in range(3):
        pair.feed_imu()
        (t,) = pair.times(0.4 + 0.1 * step)
        offsets.append(ga.aux_state(ha)[0])
        z = sim.traj.pos(t) + sim.traj.R_ItoG(t) @ arm_true
        gb.propagate(t)
        ob = gb.position_fix_lever_arm(z, hb, R3, chi2_mult=INF)
        assert ob["applied"]
        assert ga.feed_measurement_position(t, z, R3, aux_handle=ha, chi2_mult=INF)
        pair.frame()
        _same_results(ga.position_results(), [ob], [t])
        pair.close_enough("aux lever arm %d" % step)
        assert ga.aux_state(ha)[0] == gb.aux_state(hb)[0]
    arm = ga.aux_state(ha)[1]
    print("FIXARM offsets %s arm error %.4f -> %.4f" % (offsets, np.linalg.norm(arm0 - arm_true),
                                                       np.linalg.norm(arm - arm_true)))
    assert len(set(offsets)) > 1, "no clone was marginalized in front of the variable"
    assert np.linalg.norm(arm - arm_true) < np.linalg.norm(arm0 - arm_true)
    for m, h in ((ga, ha), (gb, hb)):
        m.remove_state(h)
    assert ga.aux_count() == (0, 0)


# ---- 6 ----
def test_drops_refusals_gate_and_feed_time_errors(pair):
    import uvio_amd as U
    from uvio_amd import _native as N
    ga, gb, sim = pair.ga, pair.gb, pair.sim
    s = np.array([0.2, -0.05, 0.1])

    def truth(t):
        return sim.traj.pos(t) + sim.traj.R_ItoG(t) @ s

    # a fix overtaken by uvio_hp_propagate, and a fix at the frame time: dropped, A stays what B is
    pair.feed_imu()
    ta, tp, t_frame = pair.times(0.3, 0.5, 1.0)
    assert ga.feed_measurement_position(ta, truth(ta), R3, p_SinI=s)
    for m in (ga, gb):
        m.propagate(tp)
    assert not ga.feed_measurement_position(tp, truth(tp), R3, p_SinI=s)  # not after the state time: not kept
    assert ga.feed_measurement_position(t_frame, truth(t_frame), R3, p_SinI=s)
    pair.frame()
    assert ga.position_results() == [{"t": ta, "chi2": 0.0, "status": 2}, {"t": t_frame, "chi2": 0.0, "status": 2}]
    assert pair.identical()

    # an aux handle that died after queueing: refused; a fix 10 m off: gated.  Neither changes P or x: B only propagates
    pair.feed_imu()
    ta, tb = pair.times(0.4, 0.6)
    ha, hb = ga.add_state(s, PRIOR3), gb.add_state(s, PRIOR3)
    assert ga.feed_measurement_position(ta, truth(ta), R3, aux_handle=ha)
    assert ga.feed_measurement_position(tb, truth(tb) + np.array([10.0, 0.0, 0.0]), R3, p_SinI=s)
    ga.remove_state(ha)
    gb.remove_state(hb)
    for t in (ta, tb):
        gb.propagate(t)
    pair.frame()
    res = ga.position_results()
    assert [(r["t"], r["status"]) for r in res] == [(ta, 3), (tb, 1)], res
    assert res[1]["chi2"] > U.chi2_95(3)
    assert pair.identical()

    # feed-time refusals leave the queue and the state untouched
    pair.feed_imu()
    (t,) = pair.times(0.5)
    x0, P0 = ga.get_state_vector()[0], ga.get_cov()
    z = truth(t)
    with pytest.raises(ValueError):
        ga.feed_measurement_position(t, z[:2], np.eye(2))
    bad = [dict(z=np.zeros(4), R=np.eye(4), Cm=np.zeros((4, 3))),
           dict(z=[np.nan, 0.0, 0.0]), dict(t=float("nan")), dict(R=np.triu(np.full((3, 3), np.inf))),
           dict(R=np.diag([1.0, 0.0, 1.0])), dict(R=np.diag([1.0, -1.0, 1.0])), dict(Cm=np.full((3, 3), np.nan)),
           dict(p_SinI=[0.0, np.inf, 0.0]), dict(chi2_mult=0.0), dict(chi2_mult=-1.0), dict(chi2_mult=float("nan")),
           dict(aux_handle=ha), dict(aux_handle=12345)]
    h1 = ga.add_state([0.5], [[1.0]])  # a live variable of the wrong dimension
    bad.append(dict(aux_handle=h1))
    for over in bad:
        kw = dict(t=t, z=z, R=R3, p_SinI=s)
        kw.update(over)
        with pytest.raises(RuntimeError, match="E_ARG"):
            ga.feed_measurement_position(kw.pop("t"), kw.pop("z"), kw.pop("R"), **kw)
    ga.remove_state(h1)
    lib, dp = N.load(), C.POINTER(C.c_double)
    q = C.c_int(-3)
    I3, zc, Rc, sc = (np.ascontiguousarray(a, dtype=np.float64) for a in (np.eye(3), z, R3, s))
    ptrs = [a.ctypes.data_as(dp) for a in (I3, zc, Rc, sc)]
    for k in range(4):  # a null C, z, R or p_SinI
        a = list(ptrs)
        a[k] = None
        assert lib.uvio_hp_feed_position(ga._h, t, 3, a[0], a[1], a[2], 3, a[3], 0, 1.0, C.byref(q)) == N.E_ARG
    assert lib.uvio_hp_feed_position(ga._h, t, 3, ptrs[0], ptrs[1], ptrs[2], 2, ptrs[3], 0, 1.0,
                                     C.byref(q)) == N.E_ARG  # ldr < r
    # the queue holds 256 fixes; all of these sit at the frame time, where the frame drops them without device work
    (t_frame,) = pair.times(1.0)
    for k in range(256):
        assert ga.feed_measurement_position(t_frame, z, R3, p_SinI=s)
    with pytest.raises(RuntimeError, match="E_CAPACITY"):
        ga.feed_measurement_position(t, z, R3, p_SinI=s)
    n = C.c_int(0)
    assert np.array_equal(ga.get_state_vector()[0], x0) and np.array_equal(ga.get_cov(), P0)
    pair.frame()
    res = ga.position_results()
    assert len(res) == 256 and all(r["status"] == 2 and r["t"] == t_frame for r in res)
    assert lib.uvio_hp_get_position_results(ga._h, None, None, None, 255, C.byref(n)) == N.E_CAPACITY and n.value == 256
    assert pair.identical()
    # the queue is empty again: a fix is taken and applied
    pair.feed_imu()
    (t,) = pair.times(0.5)
    zb, ob = _explicit_fix(gb, t, [0.01, 0.0, -0.01], s, R3)
    assert ga.feed_measurement_position(t, zb, R3, p_SinI=s)
    pair.frame()
    _same_results(ga.position_results(), [ob], [t])


# ---- 3 ----
def test_fix_interleaved_with_uwb_messages(euroc_yaml):
    """What the explicit path cannot express: a buffered UWB message older than a fix the caller propagated to is
    skipped by the frame, so UWB and an explicit fix between two frames do not combine.  Buffered, they do."""
    import uvio_amd as U
    opts, anchors, sim, (ga, gb) = _uwb_setup(euroc_yaml, lambda op: (U.VioManager(op), U.VioManager(op)))
    last = {}
    sim.run([ga, gb], n_frames=10, on_frame=lambda nf, t: last.update(t=t),
            after_init=lambda m: m.try_to_initialize_uwb_anchors(anchors))
    p = Pair(opts, sim, ga, gb, last["t"])
    assert p.identical(), "two handles on one stream differ: nothing below can be compared"
    p.feed_imu()
    t1, t2, t3 = p.times(0.25, 0.5, 0.75)
    s = np.array([0.2, -0.05, 0.1])
    r1 = _true_range(sim, opts, anchors[3], t1) + 0.03
    r3 = _true_range(sim, opts, anchors[0], t3) + 0.03
    gb.propagate(t1)
    assert gb.uwb_update_single(t1, anchors[3].id, r1), "a consistent range was gated"
    z, of = _explicit_fix(gb, t2, [0.01, -0.004, 0.006], s, R3)
    assert of["applied"]
    gb.propagate(t3)
    assert gb.uwb_update_single(t3, anchors[0].id, r3), "a consistent range was gated"
    # A: fed out of time order on purpose, the frame sorts them
    ga.feed_measurement_uwb(t3, [anchors[0].id], [r3])
    assert ga.feed_measurement_position(t2, z, R3, p_SinI=s)
    ga.feed_measurement_uwb(t1, [anchors[3].id], [r1])
    p.frame()
    _same_results(ga.position_results(), [of], [t2])
    # both ranges were applied on A: it agrees with B, on which both were
    p.close_enough("uwb, fix, uwb")
    ga.close()
    gb.close()


# ---- 7 ----
def test_cpp_facade_queues_and_refuses_on_the_device(tmp_path):
    from test_facade_fix import CFG, build_check, run_env
    exe = build_check(tmp_path)
    r = subprocess.run([exe, CFG, "gpu"], capture_output=True, text=True, timeout=120, env=run_env())
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "refused: code -1" in r.stdout and "FIX ok" in r.stdout
