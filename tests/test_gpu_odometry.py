"""What the ROS node reads after every message, on the GPU: marginal covariance blocks (uvio_hp_get_marginal_cov),
the IMU-rate odometry (uvio_hp_odometry_enable / uvio_hp_fast_state_propagate) and the frame's MSCKF features
(uvio_hp_get_good_features_msckf), on the EuRoC configuration with the small simulated stream of smoke().

The odometry is compared with tests/fastprop_ref.py, the numpy restatement of Propagator::fast_state_propagate.
The restatement keeps its own cache, refreshed from the device's getters after exactly the calls after which the
reference invalidates its cache (a frame that reaches its update stage or ends in a zero-velocity update); state
and covariance agree within 1e-10 relative at every query, the bound of the project's lock-step tests."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import fastprop_ref as FR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EUROC = os.path.join(ROOT, "configs", "euroc_mav", "estimator_config.yaml")
TOL = 1e-10
V_IMU, V_VEC, V_QUAT, V_POSE = 0, 1, 2, 3


def _opts(**ov):
    import uvio_amd as U
    kw = dict(max_msckf_in_update=60, max_slam_features=10, max_slam_in_update=5, dt_slam_delay=0.3)
    kw.update(ov)
    return U.load_options(EUROC, **kw)


def _sim(opts, n, **kw):
    from uvio_amd.sim import SimStream
    args = dict(duration=n / opts.track_frequency + 1.2, seed=7, spawn=60, frac_long=0.3)
    args.update(kw)
    return SimStream(opts, **args)


def _drive(g, sim, n_frames, after_imu=None, after_frame=None, feed=None):
    """SimStream.run's loop with a hook after every IMU feed; feed(nf, t, i): a custom camera feed"""
    nf = 0
    for kind, t, i in sim.events():
        if t < sim.t0 - 0.4:
            continue
        if kind == "imu":
            g.feed_measurement_imu(t, sim.wm[i], sim.am[i])
            if after_imu is not None:
                after_imu(t, sim.wm[i], sim.am[i])
        elif kind == "cam":
            if t <= sim.t0:
                continue
            if feed is not None:
                feed(nf, t, i)
            else:
                g.feed_measurement_simulation(t, list(range(sim.K)), sim.frames[i])
            nf += 1
            if after_frame is not None:
                after_frame(nf, t)
            if nf >= n_frames:
                break
    return nf


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _vlen(kind, size):
    return {V_IMU: 16, V_QUAT: 4, V_POSE: 7}.get(int(kind), int(size))


def _refresh(fp, g, opts):
    """the restatement's cache from the device's getters: what Propagator.cpp:144-150 reads from the state"""
    t, est = g.get_imu_state()
    x, meta = g.get_state_vector()
    assert meta[0][0] == V_IMU and meta[0][1] == 0
    P = g.get_cov()
    # the state's variables in order (State.cpp:28-166): IMU, [Dw, Da, (Tg), R_GYROtoIMU | R_ACCtoIMU], [dt], ...
    off, vals = 0, []
    for kind, cid, size in meta:
        vals.append(x[off:off + _vlen(kind, size)])
        off += _vlen(kind, size)
    cal = dict(imu_model=opts.imu_model, dw=list(opts.imu_dw), da=list(opts.imu_da), tg=list(opts.imu_tg),
               q_acc=list(opts.q_ACCtoIMU), q_gyro=list(opts.q_GYROtoIMU))
    k = 1
    if opts.do_calib_imu_intrinsics:
        cal["dw"], cal["da"] = vals[k], vals[k + 1]
        k += 2
        if opts.do_calib_imu_g_sensitivity:
            cal["tg"] = vals[k]
            k += 1
        cal["q_gyro" if opts.imu_model == 0 else "q_acc"] = vals[k]
        k += 1
    t_off = opts.calib_camimu_dt
    if opts.do_calib_camera_timeoffset:
        assert meta[k][2] == 1
        t_off = float(vals[k][0])
    fp.refresh(t, est, P[0:15, 0:15], t_off, FR.Calib(**cal))


def _noise(opts):
    return FR.Noise(opts.sigma_w, opts.sigma_a, opts.sigma_wb, opts.sigma_ab, opts.gravity_mag)


def _reached_update(g, opts):
    """the frame ran its update stage (VioManager.cpp:526, 543) or ended in a zero-velocity update (:230, :303)"""
    return len(g.get_clone_times()) >= min(opts.max_clone_size, 5) or g.get_timing()["zupt"] == 1


# ---------------------------------------------------------------------------------------------------------------
# 1. marginal covariances
@pytest.fixture(scope="module")
def after_8_frames():
    import uvio_amd as U
    opts = _opts()
    sim = _sim(opts, 8)
    g = U.VioManager(opts, device=0)
    g.initialize_with_gt(sim.gt_state(sim.t0))
    assert _drive(g, sim, 8) == 8
    yield g, opts
    g.close()


def _blocks(g):
    _, meta = g.get_state_vector()
    var = [(int(cid), int(size)) for _, cid, size in meta]
    clones = [(int(cid), int(size)) for kind, cid, size in meta if kind == V_POSE and cid >= 15 + 1]
    N = g.cov_dim()
    scalar = [v for v in var if v[1] == 1][:1] or [(4, 1)]
    m65, tot = [], 0
    for v in var:
        if tot + v[1] <= 65:
            m65.append(v)
            tot += v[1]
    if tot < 65:
        m65.append((N - (65 - tot), 65 - tot))  # part of the last variable fills the rest
    clone = clones[-1]
    return N, {
        "scalar": scalar,
        "imu": [(0, 15)],
        "imu_pose": [(0, 6)],
        "clone_then_imu": [clone, (0, 15)],
        "repeated": [(0, 15), clone, (0, 15)],
        "m65": m65,
        "full": var,
    }


@pytest.mark.parametrize("which", ["scalar", "imu", "imu_pose", "clone_then_imu", "repeated", "m65", "full"])
def test_marginal_cov_equals_full_covariance_gather(after_8_frames, which):
    g, _ = after_8_frames
    N, lists = _blocks(g)
    blocks = lists[which]
    idx = np.concatenate([np.arange(c, c + s) for c, s in blocks])
    m = len(idx)
    assert {"scalar": 1, "imu": 15, "imu_pose": 6, "m65": 65, "full": N}.get(which, m) == m
    if which == "clone_then_imu":
        assert blocks[0][0] > blocks[1][0] and m == 21
    if which == "full":
        assert N % 64 != 0 and N > 65
    P = g.get_cov()
    want = P[np.ix_(idx, idx)]
    got = g.get_marginal_cov(blocks)
    assert got.shape == (m, m) and got.tobytes() == want.tobytes()
    # a leading dimension above m: the padding stays as it was
    ld = m + 3
    out = np.full((m, ld), -7.0)
    from uvio_amd import _native as N_
    ids = np.array([b[0] for b in blocks], dtype=np.int32)
    sizes = np.array([b[1] for b in blocks], dtype=np.int32)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    rc = N_.load().uvio_hp_get_marginal_cov(g._h, len(blocks), ids.ctypes.data_as(ip), sizes.ctypes.data_as(ip),
                                            out.ctypes.data_as(dp), ld)
    assert rc == 0
    assert out[:, :m].tobytes() == want.tobytes() and np.all(out[:, m:] == -7.0)


def test_marginal_cov_argument_errors_leave_out_untouched(after_8_frames):
    from uvio_amd import _native as N_
    g, _ = after_8_frames
    lib = N_.load()
    N = g.cov_dim()
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    out = np.full((700, 700), -7.0)

    def call(ids, sizes, ld, nvar=None, out_=out, null=None):
        ids = np.array(ids, dtype=np.int32)
        sizes = np.array(sizes, dtype=np.int32)
        a = [g._h, len(ids) if nvar is None else nvar, ids.ctypes.data_as(ip), sizes.ctypes.data_as(ip),
             out_.ctypes.data_as(dp) if out_ is not None else None, ld]
        if null is not None:
            a[null] = None
        return lib.uvio_hp_get_marginal_cov(*a)

    assert call([0], [15], 700, null=0) == N_.E_ARG      # no handle
    assert call([0], [15], 700, null=2) == N_.E_ARG      # null ids
    assert call([0], [15], 700, null=3) == N_.E_ARG      # null sizes
    assert call([0], [15], 700, out_=None) == N_.E_ARG   # null out
    assert call([0], [15], 700, nvar=-1) == N_.E_ARG
    assert call([0, 15], [15, 0], 700) == N_.E_ARG       # a size below 1
    assert call([-1], [3], 700) == N_.E_ARG              # a block outside [0, N)
    assert call([N - 2], [3], 700) == N_.E_ARG
    assert call([N], [1], 700) == N_.E_ARG
    assert call([0, 15], [15, 6], 20) == N_.E_ARG        # ld < m
    assert call([0] * 40, [15] * 40, 700) == N_.E_CAPACITY  # m = 600 above the covariance capacity
    assert call([0], [15], 700, nvar=0) == 0             # nothing asked: nothing done
    assert np.all(out == -7.0)
    assert call([N - 1], [1], 700) == 0 and out[0, 0] == g.get_cov()[N - 1, N - 1]


# ---------------------------------------------------------------------------------------------------------------
# 2. odometry in lock-step with the restatement
def _lockstep(opts, sim, n):
    import uvio_amd as U
    g = U.VioManager(opts, device=0)
    try:
        g.initialize_with_gt(sim.gt_state(sim.t0))
        g.enable_odometry(True)
        fp = FR.FastPropagator(_noise(opts))
        _refresh(fp, g, opts)
        imu, worst = [], {"state": 0.0, "cov": 0.0}
        count = {"query": 0, "ok": 0, "refresh": 0, "skipped_early": 0, "zupt": 0}
        totals = []

        def after_imu(t, wm, am):
            imu.append((t, np.array(wm, dtype=float), np.array(am, dtype=float)))
            got, want = g.fast_state_propagate(t), fp.query(imu, t)
            count["query"] += 1
            assert (got is None) == (want is None), (t, got is None)
            if got is None:
                return
            count["ok"] += 1
            es, ec = _rel(got[0], want[0]), _rel(got[1], want[1])
            worst["state"], worst["cov"] = max(worst["state"], es), max(worst["cov"], ec)
            assert es < TOL and ec < TOL, (count, t, es, ec)

        def after_frame(nf, t):
            totals.append(g.get_timing()["total"])
            count["zupt"] += g.get_timing()["zupt"]
            if _reached_update(g, opts):
                _refresh(fp, g, opts)
                count["refresh"] += 1
            elif count["refresh"] == 0:
                count["skipped_early"] += 1  # returned before its update stage: the device must not refresh either

        assert _drive(g, sim, n, after_imu=after_imu, after_frame=after_frame) == n
        print("odometry lock-step:", count, worst, "mean total per frame %.1f us" % (1e6 * np.mean(totals)))
        return count, worst
    finally:
        g.close()


def test_odometry_lockstep_with_restatement():
    opts = _opts()
    n = 18
    count, worst = _lockstep(opts, _sim(opts, n), n)
    assert count["ok"] >= 100 and count["refresh"] >= 10, count
    # the first frames return before their update stage: the cache kept chaining from the initial state there
    assert count["skipped_early"] >= 3, count
    assert worst["state"] < TOL and worst["cov"] < TOL


def test_odometry_lockstep_zero_velocity_frames_refresh():
    """the resting stream of tests/test_gpu_zupt_retri.py: the zero-velocity frames refresh the cache"""
    opts = _opts(try_zupt=1, zupt_only_at_beginning=1, zupt_chi2_multipler=1.0, zupt_max_velocity=0.1,
                 zupt_noise_multiplier=10.0, zupt_max_disparity=0.5)
    n = 22  # 20 frames at rest, two moving
    count, worst = _lockstep(opts, _sim(opts, n, seed=5, sigma_pix=0.3, static_for=1.0), n)
    assert count["zupt"] >= 5, count
    assert count["ok"] >= 100 and count["refresh"] >= 10, count
    assert worst["state"] < TOL and worst["cov"] < TOL


# ---------------------------------------------------------------------------------------------------------------
# 3. off by default, harmless when on
def test_odometry_off_by_default_and_does_not_change_the_filter():
    import uvio_amd as U
    opts = _opts()
    n = 18
    sim = _sim(opts, n)
    final, totals = {}, {}
    for on in (False, True):
        g = U.VioManager(opts, device=0)
        try:
            g.initialize_with_gt(sim.gt_state(sim.t0))
            with pytest.raises(RuntimeError, match="E_STATE"):
                g.fast_state_propagate(sim.t0 + 0.01)
            if on:
                g.enable_odometry(True)
            tot = []
            q = (lambda t, wm, am: g.fast_state_propagate(t)) if on else None
            assert _drive(g, sim, n, after_imu=q, after_frame=lambda nf, t: tot.append(g.get_timing()["total"])) == n
            final[on] = (g.get_state_vector()[0].tobytes(), g.get_cov().tobytes())
            totals[on] = 1e6 * float(np.mean(tot[5:]))
            if on:
                g.enable_odometry(False)
                with pytest.raises(RuntimeError, match="E_STATE"):
                    g.fast_state_propagate(sim.cam_t[n - 1])
        finally:
            g.close()
    print("mean total per frame (frames 6..%d): cache off %.1f us, cache on and queried %.1f us" % (n, totals[False], totals[True]))
    assert final[True][0] == final[False][0], "the state vector differs with the odometry cache on"
    assert final[True][1] == final[False][1], "the covariance differs with the odometry cache on"


def test_odometry_refused_before_initialization():
    import uvio_amd as U
    g = U.VioManager(_opts(), device=0)
    try:
        g.enable_odometry(True)
        with pytest.raises(RuntimeError, match="E_STATE"):
            g.fast_state_propagate(1.0)
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. beside the feeds
def test_odometry_queries_from_a_second_thread_beside_the_feeds():
    import uvio_amd as U
    opts = _opts()
    n = 10
    sim = _sim(opts, n)
    g = U.VioManager(opts, device=0)
    try:
        g.initialize_with_gt(sim.gt_state(sim.t0))
        g.enable_odometry(True)
        latest = {"t": sim.t0, "stop": False}
        res = {"calls": 0, "accepted": 0, "errors": []}
        imu = []

        def worker():
            while not latest["stop"]:
                try:
                    r = g.fast_state_propagate(latest["t"])  # ctypes releases the GIL inside the call
                except Exception as ex:  # noqa: BLE001
                    res["errors"].append(repr(ex))
                    return
                res["calls"] += 1
                if r is not None:
                    res["accepted"] += 1
                    if not (np.all(np.isfinite(r[0])) and np.all(np.isfinite(r[1])) and
                            abs(np.linalg.norm(r[0][0:4]) - 1.0) < 1e-12):
                        res["errors"].append("bad result at call %d" % res["calls"])
                        return

        def after_imu(t, wm, am):
            imu.append((t, np.array(wm, dtype=float), np.array(am, dtype=float)))
            latest["t"] = t

        th = threading.Thread(target=worker)
        th.start()
        try:
            assert _drive(g, sim, n, after_imu=after_imu) == n
        finally:
            latest["stop"] = True
            th.join()
        assert not res["errors"], res["errors"][:3]
        assert res["calls"] > 0 and res["accepted"] > 0, res
        # one serial query from a fresh snapshot of the final state equals the restatement refreshed from it
        g.enable_odometry(True)
        fp = FR.FastPropagator(_noise(opts))
        _refresh(fp, g, opts)
        got, want = g.fast_state_propagate(imu[-1][0]), fp.query(imu, imu[-1][0])
        assert got is not None and want is not None
        assert _rel(got[0], want[0]) < TOL and _rel(got[1], want[1]) < TOL
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. good features
def _kept(g):
    ids, pG, st, _ = g.debug_last_msckf()
    return pG[st == 0]


def test_good_features_equal_the_kept_msckf_features():
    import uvio_amd as U
    opts = _opts()
    n = 18
    sim = _sim(opts, n)
    g = U.VioManager(opts, device=0)
    try:
        g.initialize_with_gt(sim.gt_state(sim.t0))
        assert g.get_good_features_msckf().shape == (0, 3)
        seen = []

        def after_frame(nf, t):  # every frame's first camera id is 0: the list is this frame's
            good, kept = g.get_good_features_msckf(), _kept(g)
            assert good.tobytes() == kept.tobytes(), nf
            seen.append(len(good))

        assert _drive(g, sim, n, after_frame=after_frame) == n
        assert max(seen) > 10, seen
    finally:
        g.close()


def test_good_features_accumulate_over_a_mono_camera_pair():
    """two mono cameras fed in turn (VioManager.cpp:555-570): camera 0's frame clears the list, camera 1's
    appends to it"""
    import uvio_amd as U
    opts = _opts(use_stereo=0, max_slam_features=0)
    assert opts.num_cameras == 2
    n = 40
    sim = _sim(opts, n, cam_rate=2 * opts.track_frequency, duration=n / (2 * opts.track_frequency) + 1.2)
    g = U.VioManager(opts, device=0)
    try:
        g.initialize_with_gt(sim.gt_state(sim.t0))
        expected = [np.zeros((0, 3))]
        accumulated = []

        def feed(nf, t, i):
            cam = i % 2
            g.feed_measurement_simulation(t, [cam], [sim.frames[i][cam]])
            if len(g.get_clone_times()) >= min(opts.max_clone_size, 5):  # the frame ran its MSCKF update
                kept = _kept(g)
                expected[0] = kept if cam == 0 else np.concatenate([expected[0], kept])
                if cam == 1 and len(kept) and len(expected[0]) > len(kept):
                    accumulated.append(nf)
            assert g.get_good_features_msckf().tobytes() == expected[0].tobytes(), (nf, cam)

        assert _drive(g, sim, n, feed=feed) == n
        assert len(accumulated) >= 3, accumulated
    finally:
        g.close()
