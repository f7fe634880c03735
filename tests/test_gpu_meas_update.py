"""The caller's own measurement on the device: uvio_hp_ekf_update_r (dense R behind a chi2 gate on a standalone
covariance), uvio_hp_measurement_update and uvio_hp_propagate on a handle.

1. Numerics: the dense-R update against the extended-precision reference (tests/meas_ref.py) at the dispatch
   edges of k_ekf_fact<W, LDS, true> (meas_ref.SHAPES: panel waves 1 / 2 / 3 / 5, the factor in LDS up to r = 137 and in
   global memory from 138, N around the 16-row tiles of P), R dense and graded over four orders of magnitude, no gate.
   P exactly symmetric, and in ekf_ref.scaled_err / scaled_dx_err units
       e_dev <= RATIO * max(e_f64, 16 * 2^-52)
   with e_f64 the float64 NumPy comparator's error against the same reference in the same test.
   RATIO = 16: 4 x the worst measured ratio, rounded up to a power of two (the procedure of
   tests/test_gpu_ekf_paths.py, whose information-form paths need 64).  Measured on MI355X over the ten cases:
       dx   2.33  N272-n255-r255   (device 1.08e-13, float64 4.64e-14)
       P+   0.80  N272-n255-r255   (device 2.86e-15, float64 2.26e-15; below the floor 16 * 2^-52 up to r = 17)
   The device sums its MFMA chains in another order than NumPy and multiplies by the explicit inverse factor where
   NumPy substitutes, so a small constant over the comparator is expected.  chi2 agrees with the reference to
   1.4e-14 (relative) at r = 138.
2. Bit identity with uvio_hp_ekf_update for R = sigma2 I: the new path reuses M, the factor and the P update.
3. The gate: chi2 within 1e-10 of the reference's, the threshold applied on both sides of it.
4. Refusals.
5. A UWB range through measurement_update against the oracle's UpdaterUWB::update_single.
6. position_fix and a 6-row pose fix with dense R on a 10-frame snapshot, with the bound of 1 (measured: P+ ratio
   0.15 and 0.09, dx 0.02 and 0.05: device and comparator both within 6e-16 of the reference).
7. uvio_hp_propagate + uwb_update_single reproduce feed_uwb's path to the bit.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ekf_ref as E  # noqa: E402
import meas_ref as M  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not E.HAVE_EXTENDED, reason=E.REASON)]

RATIO = 16.0
FLOOR = 16 * 2.0 ** -52
INF = float("inf")


@functools.lru_cache(maxsize=None)
def _case(s):
    """the case of one shape with its reference (longdouble) and comparator (float64) results, computed once"""
    k = M.graded_R_case(*s, seed=M.shape_seed(s))
    for a in k:
        a.setflags(write=False)
    return k, M.ekf_update_R_ref(*k), M.ekf_update_R_ref(*k, dtype=np.float64)


def _check_against_reference(tag, P0, Pg, dxg, ref, cmp64):
    Pr, dxr, _ = ref
    P6, dx6, _ = cmp64
    e_dev, e_64 = E.scaled_err(Pg, Pr, P0), E.scaled_err(P6, Pr, P0)
    x_dev, x_64 = E.scaled_dx_err(dxg, dxr, P0), E.scaled_dx_err(dx6, dxr, P0)
    print("MEASPATH %s P dev %.3e f64 %.3e ratio %.2f dx dev %.3e f64 %.3e ratio %.2f" %
          (tag, e_dev, e_64, e_dev / max(e_64, FLOOR), x_dev, x_64, x_dev / max(x_64, FLOOR)))
    assert np.array_equal(Pg, Pg.T)
    assert e_dev <= RATIO * max(e_64, FLOOR), (e_dev, e_64)
    assert x_dev <= RATIO * max(x_64, FLOOR), (x_dev, x_64)


# ---- 1 ----
@pytest.mark.parametrize("s", M.SHAPES, ids=M.shape_id)
def test_dense_R_update_against_extended_reference(s):
    import uvio_amd as U
    k, ref, cmp64 = _case(tuple(s))
    Pg, dxg, chi2, applied = U.ekf_update_R(k.P, k.idx, k.H, k.res, k.R)
    assert applied and np.isfinite(chi2)
    _check_against_reference(M.shape_id(s), k.P, Pg, dxg, ref, cmp64)
    # the triangle below R's diagonal is never read: NaN there, and a leading dimension wider than r
    Rw = np.full((s[2], s[2] + 3), np.nan)
    Rw[:, :s[2]] = np.triu(k.R) + np.tril(np.full_like(k.R, np.nan), -1)
    Pn, dxn, c2n, _ = U.ekf_update_R(k.P, k.idx, k.H, k.res, Rw)
    assert np.array_equal(Pn, Pg) and np.array_equal(dxn, dxg) and c2n == chi2


# ---- 2 ----
def _direct(r):
    return [c for c in E.DIRECT_CASES if c["m"] == r and c["sigma2"] == 2.25][0]


@pytest.mark.parametrize("c", [_direct(1), _direct(111), _direct(255)], ids=E.case_id)
def test_isotropic_R_is_bit_identical_to_the_sigma2_update(c):
    """k_ekf_MS with sigma2 = 0 leaves acc + 0.0 and k_ekf_fact's dense-R instance adds R on top: (acc + 0.0) + sigma2 is the sum
    k_ekf_MS forms itself, so with no gate every later value is the same"""
    import uvio_amd as U
    k = E.graded_case(**c)
    P1, dx1 = U.ekf_update(k.P, k.idx, k.H, k.res, k.sigma2)
    P2, dx2, _, applied = U.ekf_update_R(k.P, k.idx, k.H, k.res, k.sigma2 * np.eye(c["m"]))
    assert applied
    assert np.array_equal(P1, P2) and np.array_equal(dx1, dx2)


# ---- 3 ----
@pytest.mark.parametrize("s", [(17, 6, 6), (80, 70, 64), (150, 140, 138)], ids=M.shape_id)
def test_gate_compares_the_reference_chi2(s):
    """tests/test_meas_ref.py holds the float64 comparator to the same 1e-10 on these cases"""
    import uvio_amd as U
    k, ref, _ = _case(tuple(s))
    c_ref = float(ref[2])
    Pg, dxg, chi2, applied = U.ekf_update_R(k.P, k.idx, k.H, k.res, k.R, chi2_thr=c_ref * (1 + 1e-6))
    print("MEASGATE %s chi2 dev %.17g ref %.17g rel %.2e" % (M.shape_id(s), chi2, c_ref, abs(chi2 - c_ref) / c_ref))
    assert abs(chi2 - c_ref) < 1e-10 * c_ref
    assert applied and not np.array_equal(Pg, k.P)
    Pn, dxn, chi2n, applied_n = U.ekf_update_R(k.P, k.idx, k.H, k.res, k.R, chi2_thr=c_ref * (1 - 1e-6))
    assert not applied_n and chi2n == chi2
    assert np.array_equal(Pn, k.P) and np.all(dxn == 0.0)


# ---- 4 ----
def test_standalone_refusals_touch_nothing():
    import ctypes as C
    from uvio_amd import _native as N
    import uvio_amd as U
    lib = N.load()
    k, _, _ = _case((17, 6, 6))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)

    def call(P, idx, H, res, R, ldr, thr):
        P, dx = P.copy(), np.full(P.shape[0], 7.0)
        chi2, applied = C.c_double(-3.0), C.c_int(-3)
        rc = lib.uvio_hp_ekf_update_r(P.ctypes.data_as(dp), P.shape[0], idx.ctypes.data_as(ip), H.shape[1],
                                      H.ctypes.data_as(dp), H.shape[0], res.ctypes.data_as(dp), R.ctypes.data_as(dp), ldr,
                                      thr, dx.ctypes.data_as(dp), C.byref(chi2), C.byref(applied))
        return rc, P, dx, chi2.value, applied.value

    big = np.eye(300)
    rc, P, dx, c2, ap = call(big, np.arange(40, dtype=np.int32), np.ones((256, 40)), np.zeros(256), np.eye(256), 256, INF)
    assert rc == N.E_CAPACITY and np.array_equal(P, big) and np.all(dx == 7.0) and (c2, ap) == (-3.0, -3)
    idx = np.array(k.idx)
    idx[0] = 17
    nan_res = np.array(k.res)
    nan_res[1] = np.nan
    Pk, H, res, R = np.array(k.P), np.array(k.H), np.array(k.res), np.array(k.R)
    for args in ((Pk, idx, H, res, R, 6, INF), (Pk, np.array(k.idx), H, res, R, 5, INF),
                 (Pk, np.array(k.idx), H, nan_res, R, 6, INF), (Pk, np.array(k.idx), H, res, R, 6, 0.0),
                 (Pk, np.array(k.idx), H, res, R, 6, -2.0), (Pk, np.array(k.idx), H, res, R, 6, float("nan"))):
        rc, P, dx, c2, ap = call(*args)
        assert rc == N.E_ARG and np.array_equal(P, Pk) and np.all(dx == 7.0) and (c2, ap) == (-3.0, -3)
    # S not positive definite: refused by the factor kernel's pivot check, P untouched; the valid update then runs
    S0 = H @ Pk[np.ix_(k.idx, k.idx)] @ H.T
    Rneg = -10.0 * np.max(np.diag(S0)) * np.eye(6)
    rc, P, dx, c2, ap = call(Pk, np.array(k.idx), H, res, Rneg, 6, INF)
    assert rc == N.E_ARG and np.array_equal(P, Pk) and np.all(dx == 0.0)
    with pytest.raises(RuntimeError, match="E_ARG.*positive definite"):
        U.ekf_update_R(Pk, k.idx, H, res, Rneg)
    P2, _, _, applied = U.ekf_update_R(Pk, k.idx, H, res, R)
    assert applied and not np.array_equal(P2, Pk)


# ---- the handle ----
def _feed_imu_until(sim, mgrs, t_from, t_to):
    lag = 1.0 / sim.imu_rate + 1e-9
    for i, t in enumerate(sim.imu_t):
        if t_from + lag <= t < t_to + lag:
            for m in mgrs:
                m.feed_measurement_imu(t, sim.wm[i], sim.am[i])


def _frame_index(sim, t):
    k = int(np.argmin(np.abs(sim.cam_t - t)))
    assert abs(sim.cam_t[k] - t) < 1e-9
    return k


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def _same_state(g, o, tol=1e-10):
    """tests/test_gpu_updaters.py's bound"""
    xg, mg = g.get_state_vector()
    xo, mo = o.get_state_vector()
    assert np.array_equal(mg, mo), "state layouts differ"
    assert _rel(xg, xo) < tol, _rel(xg, xo)
    assert _rel(g.get_cov(), o.get_cov()) < tol


def _uwb_setup(euroc_yaml, mgrs_factory, n=10):
    import uvio_amd as U
    from uvio_amd import _native as N
    from uvio_amd.sim import SimStream
    from test_gpu_parity import make_anchors
    opts = U.load_options(euroc_yaml, max_msckf_in_update=60, max_slam_features=0, use_uwb=1,
                          do_calib_uwb_extrinsics=1, min_dist_to_use_uwb=0.05)
    for k, v in enumerate([0.05, -0.02, 0.03]):
        opts.p_IinU[k] = v
    anchors = make_anchors(N)
    sim = SimStream(opts, duration=(n + 3) / opts.track_frequency + 1.2, seed=4, spawn=40, anchors=anchors,
                    uwb_rate=10.0, uwb_sigma=0.1)
    return opts, anchors, sim, mgrs_factory(opts)


def _true_range(sim, opts, a, t):
    p_U = sim.traj.R_ItoG(t) @ (-np.array(opts.p_IinU[:])) + sim.traj.pos(t)
    return (1 + a.dist_bias) * np.linalg.norm(np.array(a.p_AinG[:]) - p_U) + a.const_bias


# ---- 5 ----
def test_uwb_range_through_measurement_update_matches_oracle(euroc_yaml):
    """test_uwb_update_single_matches_oracle's set-up; the row is the oracle's get_uwb_jacobian_single
    (oracle.probe_uwb), fed to the engine as a caller's measurement"""
    import uvio_amd as U
    from oracle import oracle as O
    opts, anchors, sim, (g, o) = _uwb_setup(euroc_yaml, lambda op: (U.VioManager(op), O.OracleManager(op)))

    def sync():
        o.set_state(g.get_state_vector()[0], g.get_fej_vector(), g.get_cov())

    sim.run([g, o], n_frames=10, before_frame=lambda nf, t: sync(),
            after_init=lambda m: m.try_to_initialize_uwb_anchors(anchors))
    t, _ = g.get_imu_state()
    s2 = opts.uwb_sigma_range ** 2
    thr = opts.uwb_chi2_multipler * U.chi2_95(1)
    applied, gated = 0, 0
    for a in (anchors[0], anchors[3]):  # one fixed, one estimated
        true = _true_range(sim, opts, a, t)
        for rng in (true + 0.05, true + 20.0):
            sync()
            pred, H, blocks = o.probe_uwb(a.id)
            meta = {(int(m[1]), int(m[2])) for m in g.get_state_vector()[1]}
            for b in blocks:  # the IMU's pose is the head of its 15-dimensional variable
                assert (int(b[0]), int(b[1])) in meta or (int(b[0]), 15) in meta, (b, meta)
            assert sum(int(b[1]) for b in blocks) == H.shape[0] == (14 if not a.fix else 9)
            out = g.measurement_update([(int(b[0]), int(b[1])) for b in blocks], H[None, :], [rng - pred], [[s2]], thr)
            ao = o.uwb_update_single(t, a.id, rng)
            assert out["applied"] == ao
            applied += ao
            gated += not ao
            if not ao:
                assert np.all(out["dx"] == 0.0) and out["chi2"] > thr
            _same_state(g, o)
    assert applied == 2 and gated == 2
    g.close()


# ---- 4 (handle) and 6 ----
@pytest.fixture(scope="module")
def snap(euroc_yaml):
    import uvio_amd as U
    from uvio_amd.sim import SimStream
    opts = U.load_options(euroc_yaml, max_msckf_in_update=60, max_slam_features=10, max_slam_in_update=5,
                          dt_slam_delay=0.3)
    n = 10
    sim = SimStream(opts, duration=(n + 4) / opts.track_frequency + 1.2, seed=7, spawn=60, frac_long=0.3)
    g = U.VioManager(opts)
    last = {}
    sim.run(g, n_frames=n, on_frame=lambda nf, t: last.update(t=t))
    yield opts, sim, g, _frame_index(sim, last["t"])
    g.close()


def test_handle_refusals_touch_nothing(snap):
    opts, sim, g, _ = snap
    N = g.cov_dim()
    x0, P0 = g.get_state_vector()[0], g.get_cov()
    H, R, res = np.ones((3, 6)), np.eye(3), np.zeros(3)
    with pytest.raises(RuntimeError, match="E_ARG.*outside"):
        g.measurement_update([(N - 3, 6)], H, res, R)
    with pytest.raises(RuntimeError, match="E_ARG"):
        g.measurement_update([(-1, 6)], H, res, R)
    with pytest.raises(RuntimeError, match="E_ARG.*finite"):
        g.measurement_update([(0, 6)], H, [0.0, np.nan, 0.0], R)
    with pytest.raises(RuntimeError, match="E_ARG.*finite"):
        g.measurement_update([(0, 6)], H, res, np.triu(np.full((3, 3), np.inf)))
    for thr in (0.0, -1.0, float("nan")):
        with pytest.raises(RuntimeError, match="E_ARG.*threshold"):
            g.measurement_update([(0, 6)], H, res, R, thr)
    with pytest.raises(RuntimeError, match="E_CAPACITY"):
        g.measurement_update([(0, 6)], np.ones((256, 6)), np.zeros(256), np.eye(256))
    with pytest.raises(RuntimeError, match="E_CAPACITY"):
        g.measurement_update([(0, 15)] * 82, np.ones((1, 1230)), [0.0], [[1.0]])
    out = g.measurement_update([], np.zeros((0, 0)), [], np.zeros((0, 0)))
    assert not out["applied"] and np.all(out["dx"] == 0.0)
    # S not positive definite: E_ARG that says so, nothing applied, the handle stays usable
    S0 = H @ P0[:6, :6] @ H.T
    with pytest.raises(RuntimeError, match="E_ARG.*positive definite"):
        g.measurement_update([(0, 6)], H, res, -10.0 * np.max(np.diag(S0)) * np.eye(3))
    assert np.array_equal(g.get_state_vector()[0], x0) and np.array_equal(g.get_cov(), P0)
    # a NaN below R's diagonal is not read; zero rows with a positive-definite R pass and move nothing
    Rl = R + np.tril(np.full((3, 3), np.nan), -1)
    out = g.measurement_update([(0, 6)], np.zeros((3, 6)), res, Rl)
    assert out["applied"] and out["chi2"] == 0.0 and np.all(out["dx"] == 0.0)
    # (Type::update with dx = 0 still renormalizes the quaternions: the values may move in their last bit)
    assert np.max(np.abs(g.get_state_vector()[0] - x0)) < 1e-15 and np.array_equal(g.get_cov(), P0)


def _expected_values(x0, meta, dx):
    """Type::update restated: JPL quaternions move by quat_boxplus, everything else adds (kinds of
    uvio_hp_get_state_vector's meta: 0 IMU [q p v bg ba], 2 quaternion, 3 pose [q p], the others vectors).
    Returns the expected vector and the mask of the additive entries."""
    x1, additive = x0.copy(), np.ones(x0.size, bool)
    k = 0
    for kind, vid, size in meta:
        d = dx[vid:vid + size]
        if kind in (0, 2, 3):
            x1[k:k + 4] = M.quat_boxplus(x0[k:k + 4], d[:3])
            additive[k:k + 4] = False
            x1[k + 4:k + size + 1] = x0[k + 4:k + size + 1] + d[3:]
            k += size + 1
        else:
            x1[k:k + size] = x0[k:k + size] + d
            k += size
    assert k == x0.size
    return x1, additive


def _check_handle_update(tag, g, blocks, H, res, R, call):
    x0, meta = g.get_state_vector()
    f0, P0 = g.get_fej_vector(), g.get_cov()
    idx = np.concatenate([np.arange(b[0], b[0] + b[1]) for b in blocks]).astype(np.int32)
    ref = M.ekf_update_R_ref(P0, idx, H, res, R)
    cmp64 = M.ekf_update_R_ref(P0, idx, H, res, R, dtype=np.float64)
    out = call()
    assert out["applied"]
    assert abs(out["chi2"] - float(ref[2])) < 1e-10 * float(ref[2])
    _check_against_reference(tag, P0, g.get_cov(), out["dx"], ref, cmp64)
    x1, meta1 = g.get_state_vector()
    assert np.array_equal(meta, meta1)
    want, additive = _expected_values(x0, meta, out["dx"])
    assert np.array_equal(x1[additive], want[additive])
    assert np.max(np.abs(x1[~additive] - want[~additive])) < 1e-15
    assert np.array_equal(g.get_fej_vector(), f0)
    return out


def test_position_fix_and_pose_fix_with_dense_R(snap):
    import uvio_amd as U
    from uvio_amd.manager import position_fix_jacobian
    opts, sim, g, last = snap
    meta = g.get_state_vector()[1]
    imu_id = int([m for m in meta if m[0] == 0][0][1])
    rng = np.random.default_rng(5)
    # a position sensor 20 cm off the IMU, 2 cm noise with correlated axes, a fix 1 cm off the prediction
    p_SinI = np.array([0.2, -0.05, 0.1])
    A = rng.standard_normal((3, 3))
    R3 = 4e-4 * (A @ A.T / 3 + 0.1 * np.eye(3))
    x = g.get_imu_state()[1]
    pred, H3 = position_fix_jacobian(x[0:4], x[4:7], p_SinI)
    p_meas = pred + np.array([0.01, -0.004, 0.006])
    out = _check_handle_update("position_fix", g, [(imu_id, 6)], H3, p_meas - pred, R3,
                               lambda: g.position_fix(p_meas, p_SinI, R3))
    assert out["chi2"] < U.chi2_95(3)
    # a 6-row pose fix (orientation error and position, H = I) with a dense 6 x 6 R, no gate
    B = rng.standard_normal((6, 6))
    R6 = np.outer(*[np.array([1e-2] * 3 + [2e-2] * 3)] * 2) * (B @ B.T / 6 + 0.1 * np.eye(6))
    res6 = np.array([2e-3, -1e-3, 3e-3, 0.01, 0.02, -0.01])
    _check_handle_update("pose_fix", g, [(imu_id, 6)], np.eye(6), res6, R6,
                         lambda: g.measurement_update([(imu_id, 6)], np.eye(6), res6, R6))
    # the estimator goes on: two more camera frames
    for i in (last + 1, last + 2):
        _feed_imu_until(sim, [g], sim.cam_t[i - 1], sim.cam_t[i])
        g.feed_measurement_simulation(float(sim.cam_t[i]), list(range(sim.K)), sim.frames[i])
    assert abs(g.get_imu_state()[0] - sim.cam_t[last + 2]) < 1e-9
    assert np.all(np.isfinite(g.get_state_vector()[0])) and np.all(np.diag(g.get_cov()) > 0)


# ---- 7 ----
def test_propagate_then_range_updates_reproduce_feed_uwb(euroc_yaml):
    """Handle A buffers two UWB messages (one range each, so a message's range order plays no part) and processes
    them inside the next camera frame (UVioManager.cpp:178-188); handle B is moved to each message's time with
    uvio_hp_propagate and given the range with uwb_update_single, then fed the same frame."""
    import uvio_amd as U
    opts, anchors, sim, (ga, gb) = _uwb_setup(euroc_yaml, lambda op: (U.VioManager(op), U.VioManager(op)))
    last = {}
    sim.run([ga, gb], n_frames=10, on_frame=lambda nf, t: last.update(t=t),
            after_init=lambda m: m.try_to_initialize_uwb_anchors(anchors))

    def same():
        return (np.array_equal(ga.get_state_vector()[0], gb.get_state_vector()[0]) and
                np.array_equal(ga.get_cov(), gb.get_cov()))

    assert same(), "two handles on one stream differ: nothing below can be compared"
    i = _frame_index(sim, last["t"])
    t0, t1 = float(sim.cam_t[i]), float(sim.cam_t[i + 1])
    assert ga.get_imu_state()[0] == t0
    # refused: a time that is not after the state's
    xb, Pb = gb.get_state_vector()[0], gb.get_cov()
    for t in (t0, t0 - 0.01):
        with pytest.raises(RuntimeError, match="E_ORDER"):
            gb.propagate(t)
    assert np.array_equal(gb.get_state_vector()[0], xb) and np.array_equal(gb.get_cov(), Pb)
    _feed_imu_until(sim, [ga, gb], t0, t1)
    msgs = [(t0 + 0.3 * (t1 - t0), anchors[3]), (t0 + 0.65 * (t1 - t0), anchors[0])]
    msgs = [(tu, a, _true_range(sim, opts, a, tu) + 0.03) for tu, a in msgs]
    for tu, a, r in msgs:
        ga.feed_measurement_uwb(tu, [a.id], [r])
    for tu, a, r in msgs:
        gb.propagate(tu)
        assert gb.get_imu_state()[0] == tu
        assert gb.uwb_update_single(tu, a.id, r), "a consistent range was gated"
    assert not same()
    for m in (ga, gb):
        m.feed_measurement_simulation(t1, list(range(sim.K)), sim.frames[i + 1])
    assert ga.get_imu_state()[0] == t1
    assert same()
    ga.close()
    gb.close()
