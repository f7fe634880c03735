"""Caller-defined ("auxiliary") state variables on the device: k_aux_append, k_aux_init / k_aux_init_own and k_aux_walk
through their standalone twins, and uvio_hp_aux_add / _add_from_measurement / _get / _remove on a handle.

1. Kernel shapes at the dispatch edges (SHAPE_N x d in (1, 3, 8) x SHAPE_n, ld > N + d, unsorted non-contiguous
   columns, the lower triangles of the prior and of R poisoned with NaN): N around k_aux_init's 4 rows per workgroup
   (3, 4, 5), the 16 / 64 / 256 boundaries of the other covariance kernels and the largest state 1215 - d; n around
   one and two 64-lane rounds of the row sums (63, 64, 65, 127, 128, 129); (N + d) d around k_aux_append's 256-thread
   workgroup (d = 8: N = 23, 24, 25); 63, 64, 65 walking components around k_aux_walk's 64-thread workgroup.
   Append and walk are bit-identical to the float64 replay (tests/aux_ref.py), [0, N)^2 keeps its digest and the
   padding beyond N + d its bytes.  k_aux_init, in the correlation units of the augmented covariance:
       e_dev <= RATIO * max(e_f64, 16 * 2^-52)
   with e_f64 the float64 comparator's error against the same longdouble reference.
   RATIO = 4: 4 x the worst measured ratio, rounded up to a power of two.  Measured on MI355X over the 378 shapes:
   worst ratio 1.00 (d = 1: 0.54, its errors lie below the floor) -- the kernels round every product and sum by
   itself in the documented order, and the device's rows and columns were bit-identical to the comparator's in every
   case, so e_dev = e_f64; the largest of both: 1.73e-12 at N3-d8-n1, 1.07e-12 at N15-d8-n63.  The margin covers a
   different summation tree at shapes not swept.  The handle's aux_add_from_measurement (5): ratio 0.07 (device
   2.4e-16, comparator 2.0e-16; H_aux^-1 is formed by the library there, in float64).
2. An idle passenger (a 3-vector, sigma = 0, never measured) changes nothing on a 10-frame stream.
3. The random walk over camera frames, zero-velocity frames and uvio_hp_propagate calls is the float64 replay's, bit
   for bit.
4. position_fix_lever_arm step by step against the longdouble EKF reference (tests/test_gpu_meas_update.py's
   _check_handle_update and bound).
5. aux_add_from_measurement on the snapshot, a measurement_update naming the new block, aux_remove.
6. Refusals on a live handle touch nothing.
7. The C++ facade (tests/cpp/facade_aux_check.cpp) on the device.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import aux_ref as A  # noqa: E402
import ekf_ref as E  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not E.HAVE_EXTENDED, reason=E.REASON)]

RATIO = 4.0
FLOOR = 16 * 2.0 ** -52
PAD = -7.25  # uvio_amd.manager._padded's filler

SHAPE_N = [1, 3, 4, 5, 15, 16, 17, 23, 24, 25, 63, 64, 65, 255, 256, 257]
SHAPE_n = [1, 6, 63, 64, 65, 127, 128, 129]
DIMS = [1, 3, 8]


@functools.lru_cache(maxsize=None)
def _P(N):
    P, _ = A.spd_case(N, 700 + N)
    P.setflags(write=False)
    return P


def _poisoned(S, extra):
    """S's upper triangle in a (d, d + extra) array whose every other entry is NaN"""
    d = S.shape[0]
    W = np.full((d, d + extra), np.nan)
    W[:, :d] = np.triu(S) + np.tril(np.full((d, d), np.nan), -1)
    return W


def _untouched(buf, P, N, d):
    assert A.digest(buf[:N, :N]) == A.digest(P), "[0, N)^2 changed"
    assert np.all(buf[:, N + d:] == PAD), "padding written"


# ---- 1 ----
@pytest.mark.parametrize("d", DIMS)
def test_append_is_bit_identical_to_the_replay(d):
    import uvio_amd as U
    for N in SHAPE_N + [1215 - d]:
        P = _P(N)
        prior = A.init_case(d, d, 1, 900 + N)[5]
        want = A.append_ref(P, prior)
        for ld in (N + d, N + d + 3):
            buf = U.aux_append_p(P, _poisoned(prior, 2), ld=ld)
            got = buf[:, :N + d]
            assert np.array_equal(got, want) and not np.any(np.signbit(got[:N, N:])), (N, d, ld)
            assert np.array_equal(got, got.T)
            _untouched(buf, P, N, d)


def _walk_tables(N, dims, rng):
    """disjoint blocks of the given dims spread over [0, N) with gaps, in a shuffled order"""
    need = sum(dims) + len(dims)
    assert need <= N + 1
    ids, at = [], 0
    slack = N - sum(dims)
    for k, dm in enumerate(dims):
        gap = int(rng.integers(0, slack // len(dims) + 1)) if k else int(rng.integers(0, 2))
        gap = min(gap, N - at - sum(dims[k:]))
        at += gap
        ids.append(at)
        at += dm
    order = rng.permutation(len(dims))
    return np.array(ids, dtype=np.int32)[order], np.array(dims, dtype=np.int32)[order]


@pytest.mark.parametrize("N,dims", [(1, [1]), (15, [3]), (16, [8, 1]), (17, [3, 2, 8]), (65, [8, 3, 1, 5]),
                                    (255, [8] * 7 + [7]), (256, [8] * 8), (257, [8] * 8 + [1]), (1212, [3, 8, 1])],
                         ids=lambda v: str(v) if isinstance(v, int) else "m%d" % sum(v))
def test_walk_is_bit_identical_to_the_replay(N, dims):
    import uvio_amd as U
    rng = np.random.default_rng(50 + N)
    P = _P(N)
    ids, dm = _walk_tables(N, dims, rng)
    m = int(dm.sum())
    s2 = rng.uniform(0.0, 1e-2, m) ** 2
    s2[::5] = 0.0  # constant components inside a walking variable
    cidx = np.concatenate([np.arange(i, i + k) for i, k in zip(ids, dm)])
    for dt in (0.05000000000000071, 1.0 / 3.0, 0.0):
        want = A.walk_replay64(P, cidx, s2, dt)
        for ld in (N, N + 5):
            buf = U.aux_walk_p(P, ids, dm, s2, dt, ld=ld)
            assert np.array_equal(buf[:, :N], want), (N, dt, ld)
            assert np.all(buf[:, N:] == PAD)
            if dt == 0.0:
                assert np.array_equal(buf[:, :N], P)


@pytest.mark.parametrize("d", DIMS)
def test_init_against_extended_reference(d):
    import uvio_amd as U
    worst, identical, cases = 0.0, 0, 0
    shapes = [(N, n) for N in SHAPE_N + [1215 - d] for n in SHAPE_n]
    shapes += [(1215 - d, 1215 - d), (1215 - d, 1215), (5, 0)]
    for N, n in shapes:
        if n > N and N > 25 and n != 1215:
            continue  # (repeated columns are covered by the small N)
        P = _P(N)
        _, idx, Hx, Haux, Hinv, R = A.init_case(N, d, n, 3000 + 7 * N + n)
        if n:
            assert n == 1 or n > N or (np.any(np.diff(idx) < 0) and len(set(idx)) == n), "columns not unsorted / distinct"
        ref = A.init_ref(P, idx, Hx, Hinv, R)
        cmp64 = A.init_replay64(P, idx, Hx, Hinv, R)
        ld = N + d + 3
        buf = U.aux_init_p(P, idx, Hx, Hinv, _poisoned(R, 1), ld=ld)
        got = buf[:, :N + d]
        _untouched(buf, P, N, d)
        assert np.array_equal(got, got.T), (N, d, n)
        e_dev, e_64 = A.scaled_err_new(got, ref), A.scaled_err_new(cmp64, ref)
        ratio = e_dev / max(e_64, FLOOR)
        same = np.array_equal(got, cmp64)
        print("AUXINIT N%d-d%d-n%d dev %.3e f64 %.3e ratio %.2f bit-identical to the comparator: %s" %
              (N, d, n, e_dev, e_64, ratio, same))
        worst, identical, cases = max(worst, ratio), identical + same, cases + 1
        assert e_dev <= RATIO * max(e_64, FLOOR), (N, d, n, e_dev, e_64)
    print("AUXINIT d%d worst ratio %.3f over %d cases, %d bit-identical" % (d, worst, cases, identical))


# ---- the handle ----
from test_gpu_meas_update import _check_handle_update, _feed_imu_until, _frame_index, _rel  # noqa: E402

OVERRIDES = dict(max_msckf_in_update=60, max_slam_features=10, max_slam_in_update=5, dt_slam_delay=0.3)
PRIOR3 = np.array([[4e-2, 1e-3, -2e-3], [1e-3, 9e-2, 5e-4], [-2e-3, 5e-4, 1e-2]])


def _without(x, meta, P, aid, dim):
    """state vector, meta and covariance with the additive variable at covariance offset aid removed"""
    keep = np.ones(P.shape[0], bool)
    keep[aid:aid + dim] = False
    k, xs, ms = 0, [], []
    for kind, vid, size in meta:
        vlen = size + 1 if kind in (0, 2, 3) else size
        if vid != aid:
            xs.append(x[k:k + vlen])
            ms.append((kind, vid - dim if vid > aid else vid, size))
        else:
            assert kind == 6 and size == dim
        k += vlen
    return np.concatenate(xs), np.array(ms, dtype=np.int32), P[np.ix_(keep, keep)]


# ---- 2 ----
def test_idle_passenger_changes_nothing(euroc_yaml):
    import uvio_amd as U
    from uvio_amd.sim import SimStream
    ov = dict(OVERRIDES, max_clone_size=5)  # the window fills, and clones leave, within the ten frames
    opts, opts8 = U.load_options(euroc_yaml, **ov), U.load_options(euroc_yaml, max_aux_dim=8, **ov)
    sim = SimStream(opts, duration=14 / opts.track_frequency + 1.2, seed=7, spawn=60, frac_long=0.3)
    plain, passenger, roomy = U.VioManager(opts), U.VioManager(opts8), U.VioManager(opts8)
    st = {"h": None, "ids": [], "identical": True, "checked": 0}

    def on_frame(nf, t):
        xp, mp = plain.get_state_vector()
        Pp = plain.get_cov()
        xr, mr = roomy.get_state_vector()
        assert np.array_equal(xr, xp) and np.array_equal(mr, mp) and np.array_equal(roomy.get_cov(), Pp), nf
        assert roomy.aux_count() == (0, 0)
        if nf == 3:  # three clones are in front of the variable
            st["h"] = passenger.add_state([0.3, -0.2, 0.1], PRIOR3)
            assert passenger.aux_count() == (1, 3)
        if st["h"] is None:
            return
        aid, val = passenger.aux_state(st["h"])
        st["ids"].append(aid)
        x, meta = passenger.get_state_vector()
        P = passenger.get_cov()
        assert [tuple(m) for m in meta if m[0] == 6] == [(6, aid, 3)]
        assert np.array_equal(val, [0.3, -0.2, 0.1])
        assert np.array_equal(P[aid:aid + 3, aid:aid + 3], PRIOR3), nf
        rest = np.ones(P.shape[0], bool)
        rest[aid:aid + 3] = False
        assert np.all(P[aid:aid + 3][:, rest] == 0.0) and np.all(P[rest][:, aid:aid + 3] == 0.0), nf
        x1, m1, P1 = _without(x, meta, P, aid, 3)
        assert np.array_equal(m1, mp)
        assert _rel(x1, xp) < 1e-10 and _rel(P1, Pp) < 1e-10, nf
        st["identical"] = st["identical"] and np.array_equal(x1, xp) and np.array_equal(P1, Pp)
        st["checked"] += 1

    sim.run([plain, passenger, roomy], n_frames=10, on_frame=on_frame)
    print("AUXIDLE every other entry bit-identical to the plain handle's over %d frames: %s; offsets %s" %
          (st["checked"], st["identical"], st["ids"]))
    assert st["checked"] == 8
    assert len(set(st["ids"])) > 1 and st["ids"][-1] < st["ids"][0], "the offset never moved: no clone left in front"
    for m in (plain, passenger, roomy):
        m.close()


# ---- 3 ----
def test_random_walk_over_frames_propagations_and_zero_velocity_updates(euroc_yaml):
    import uvio_amd as U
    from uvio_amd.sim import SimStream
    opts = U.load_options(euroc_yaml, max_aux_dim=8, try_zupt=1, zupt_only_at_beginning=1, zupt_chi2_multipler=1.0,
                          zupt_max_velocity=0.1, zupt_noise_multiplier=10.0, zupt_max_disparity=0.5,
                          max_msckf_in_update=100, max_slam_features=10, max_slam_in_update=5, dt_slam_delay=0.5)
    n = 16
    sim = SimStream(opts, duration=n / opts.track_frequency + 1.2, seed=5, spawn=60, frac_long=0.3, sigma_pix=0.3,
                    static_for=0.4)
    g = U.VioManager(opts)
    sigma = np.array([3e-3, 0.0125])
    prior = np.array([[1e-4, 2e-5], [2e-5, 4e-4]])
    st = {"t": None, "d": np.diag(prior).copy(), "zupt": 0, "moving": 0, "props": 0}

    def add(m):
        st["h"] = m.add_state([1.0, -1.0], prior, walk_sigma=sigma)
        st["t"] = m.get_imu_state()[0]

    def advance(tag):
        """the replay: d += fl(sigma^2 * fl(t_new - t_old)) with the handle's own state times"""
        t1 = g.get_imu_state()[0]
        dt = np.float64(t1) - np.float64(st["t"])
        assert dt > 0, tag
        st["d"] = st["d"] + (sigma * sigma) * dt
        st["t"] = t1
        aid, val = g.aux_state(st["h"])
        P = g.get_cov()
        assert np.array_equal(P[aid:aid + 2, aid:aid + 2].diagonal(), st["d"]), (tag, P[aid:aid + 2, aid:aid + 2], st["d"])
        assert P[aid, aid + 1] == prior[0, 1] and P[aid + 1, aid] == prior[0, 1]
        rest = np.ones(P.shape[0], bool)
        rest[aid:aid + 2] = False
        assert np.all(P[aid:aid + 2][:, rest] == 0.0) and np.all(P[rest][:, aid:aid + 2] == 0.0), tag
        assert np.array_equal(val, [1.0, -1.0])

    def before(nf, t):
        if nf % 2 == 0:  # uvio_hp_propagate between two frames, to a time the IMU buffer already covers
            g.propagate(st["t"] + 0.6 * (t - st["t"]))
            st["props"] += 1
            advance("propagate before frame %d" % nf)

    def after(nf, t):
        z = g.get_timing()["zupt"]
        st["zupt"] += z
        st["moving"] += 1 - z
        assert g.get_imu_state()[0] == t
        advance("frame %d (zupt %d)" % (nf, z))

    sim.run(g, n_frames=n, after_init=add, before_frame=before, on_frame=after)
    print("AUXWALK %d zero-velocity frames, %d propagate-and-clone frames, %d uvio_hp_propagate calls" %
          (st["zupt"], st["moving"], st["props"]))
    assert st["zupt"] >= 1 and st["moving"] >= 3 and st["props"] >= 5
    g.close()


# ---- the snapshot of 4, 5, 6 ----
@pytest.fixture(scope="module")
def snap8(euroc_yaml):
    import uvio_amd as U
    from uvio_amd.sim import SimStream
    opts = U.load_options(euroc_yaml, max_aux_dim=8, **OVERRIDES)
    n = 10
    sim = SimStream(opts, duration=(n + 8) / opts.track_frequency + 1.2, seed=7, spawn=60, frac_long=0.3)
    g = U.VioManager(opts)
    last = {}
    sim.run(g, n_frames=n, on_frame=lambda nf, t: last.update(t=t))
    pos = {"i": _frame_index(sim, last["t"])}

    def next_frame():
        i = pos["i"] + 1
        _feed_imu_until(sim, [g], sim.cam_t[i - 1], sim.cam_t[i])
        g.feed_measurement_simulation(float(sim.cam_t[i]), list(range(sim.K)), sim.frames[i])
        pos["i"] = i

    yield opts, sim, g, next_frame
    g.close()


def _imu_id(g):
    return int([m for m in g.get_state_vector()[1] if m[0] == 0][0][1])


# ---- 4 ----
def test_lever_arm_fix_step_by_step(snap8):
    import uvio_amd as U
    from uvio_amd.manager import position_fix_lever_arm_jacobian
    opts, sim, g, next_frame = snap8
    rng = np.random.default_rng(8)
    h = g.add_state([0.2, -0.05, 0.1], PRIOR3)
    B = rng.standard_normal((3, 3))
    R3 = 4e-4 * (B @ B.T / 3 + 0.1 * np.eye(3))
    offsets = []
    for step in range(3):
        aid, arm = g.aux_state(h)
        offsets.append(aid)
        x = g.get_imu_state()[1]
        pred, H = position_fix_lever_arm_jacobian(x[0:4], x[4:7], arm)
        p_meas = pred + np.array([0.01, -0.004, 0.006]) * (1 + 0.25 * step)
        var0 = np.diag(g.get_marginal_cov([(aid, 3)]))
        out = _check_handle_update("lever_arm_%d" % step, g, [(_imu_id(g), 6), (aid, 3)], H, p_meas - pred, R3,
                                   lambda: g.position_fix_lever_arm(p_meas, h, R3))
        assert out["chi2"] < U.chi2_95(3)
        aid1, arm1 = g.aux_state(h)
        assert aid1 == aid and np.array_equal(arm1, arm + out["dx"][aid:aid + 3])
        assert np.any(out["dx"][aid:aid + 3] != 0.0)
        var1 = np.diag(g.get_marginal_cov([(aid, 3)]))
        assert np.all(var1 < var0), (var0, var1)
        next_frame()
        next_frame()
    assert np.all(np.isfinite(g.get_state_vector()[0])) and np.all(np.diag(g.get_cov()) > 0)
    g.remove_state(h)
    assert g.aux_count() == (0, 0)


# ---- 5 ----
def test_initialize_from_a_measurement_then_use_and_remove(snap8):
    opts, sim, g, next_frame = snap8
    rng = np.random.default_rng(12)
    N0, P0 = g.cov_dim(), g.get_cov()
    imu = _imu_id(g)
    # a frame offset b seen through z = C (p_IinG + b) with a small attitude dependence: H_x over the IMU pose,
    # H_aux = C, a scaled rotation plus a perturbation (well conditioned), R dense
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    Haux = 1.5 * Q + 0.05 * rng.standard_normal((3, 3))
    Hx = np.hstack([0.3 * rng.standard_normal((3, 3)), Haux])
    B = rng.standard_normal((3, 3))
    R = A.sym_upper(1e-3 * (B @ B.T / 3 + 0.1 * np.eye(3)))
    val0, res = np.array([5.0, -3.0, 0.5]), np.array([0.02, -0.01, 0.03])
    h = g.add_state_from_measurement(val0, [(imu, 6)], Hx, Haux, res, R + np.tril(np.full((3, 3), np.nan), -1))
    aid, val = g.aux_state(h)
    assert aid == N0 and g.cov_dim() == N0 + 3 and g.aux_count() == (1, 3)
    Hinv_ld = A.inverse_ld(Haux)
    want_val = np.asarray(val0, dtype=E.LD) + Hinv_ld @ np.asarray(res, dtype=E.LD)
    assert np.max(np.abs(val - want_val)) < 1e-14 * np.max(np.abs(want_val))
    idx = np.arange(imu, imu + 6)
    P1 = g.get_cov()
    assert np.array_equal(P1[:N0, :N0], P0) and np.array_equal(P1, P1.T)
    ref = A.init_ref(P0, idx, Hx, Hinv_ld, R)
    cmp64 = A.init_replay64(P0, idx, Hx, Hinv_ld.astype(np.float64), R)
    e_dev, e_64 = A.scaled_err_new(P1, ref), A.scaled_err_new(cmp64, ref)
    print("AUXINIT handle dev %.3e f64 %.3e ratio %.2f" % (e_dev, e_64, e_dev / max(e_64, FLOOR)))
    assert e_dev <= RATIO * max(e_64, FLOOR), (e_dev, e_64)
    # a measurement naming the new block: z = C (p + b) again, a centimetre off
    Hm = np.hstack([np.zeros((3, 3)), Haux, Haux])
    _check_handle_update("aux_init_then_update", g, [(imu, 6), (aid, 3)], Hm, np.array([0.01, 0.0, -0.01]), R,
                         lambda: g.measurement_update([(imu, 6), (aid, 3)], Hm, [0.01, 0.0, -0.01], R))
    next_frame()
    # removal: marginalization copies
    aid, _ = g.aux_state(h)
    x2, m2 = g.get_state_vector()
    P2 = g.get_cov()
    g.remove_state(h)
    x3, m3, P3 = _without(x2, m2, P2, aid, 3)
    xa, ma = g.get_state_vector()
    assert g.cov_dim() == P2.shape[0] - 3 and np.array_equal(ma, m3) and np.array_equal(xa, x3)
    assert np.array_equal(g.get_cov(), P3)
    for call in (lambda: g.aux_state(h), lambda: g.remove_state(h)):
        with pytest.raises(RuntimeError, match="E_ARG.*handle"):
            call()
    assert g.aux_count() == (0, 0)
    next_frame()


# ---- 6 ----
def test_refusals_on_a_live_handle_touch_nothing(snap8, euroc_yaml):
    import uvio_amd as U
    opts, sim, g, next_frame = snap8
    N = g.cov_dim()
    imu = _imu_id(g)
    dx, dP = A.digest(g.get_state_vector()[0]), A.digest(g.get_cov())
    eye, z3 = np.eye(3), np.zeros(3)
    H6 = np.ones((3, 6))

    def from_meas(blocks=((imu, 6),), Hx=H6, Haux=eye, res=z3, R=eye, val0=z3, walk=None):
        return g.add_state_from_measurement(val0, list(blocks), Hx, Haux, res, R, walk_sigma=walk)

    with pytest.raises(RuntimeError, match="E_ARG.*singular"):
        from_meas(Haux=np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]]))
    with pytest.raises(RuntimeError, match="E_ARG.*singular"):
        from_meas(Haux=np.diag([1.0, np.nan, 1.0]))
    with pytest.raises(RuntimeError, match="E_ARG.*finite"):
        from_meas(R=np.triu(np.full((3, 3), np.nan)))
    with pytest.raises(RuntimeError, match="E_ARG.*finite"):
        from_meas(Hx=np.full((3, 6), np.inf))
    with pytest.raises(RuntimeError, match="E_ARG.*finite"):
        from_meas(res=[0.0, np.nan, 0.0])
    with pytest.raises(RuntimeError, match="E_ARG.*outside"):
        from_meas(blocks=((N - 3, 6),))
    with pytest.raises(RuntimeError, match="E_ARG.*outside"):
        from_meas(blocks=((-1, 6),))
    with pytest.raises(RuntimeError, match="E_CAPACITY.*1215"):
        from_meas(blocks=((0, 15),) * 82, Hx=np.ones((3, 1230)))
    with pytest.raises(RuntimeError, match="E_ARG.*walk_sigma"):
        from_meas(walk=[0.0, -1.0, 0.0])
    with pytest.raises(RuntimeError, match="E_ARG.*prior_cov"):
        g.add_state(z3, np.triu(np.full((3, 3), np.nan)))
    with pytest.raises(RuntimeError, match="E_ARG.*prior_cov"):
        g.add_state(z3, np.diag([1.0, 0.0, 1.0]))
    with pytest.raises(RuntimeError, match="E_ARG.*finite"):
        g.add_state([0.0, np.inf, 0.0], eye)
    with pytest.raises(RuntimeError, match="E_ARG.*dim"):
        g.add_state(np.zeros(9), np.eye(9))
    with pytest.raises(RuntimeError, match="E_ARG.*handle"):
        g.aux_state(12345)
    assert (A.digest(g.get_state_vector()[0]), A.digest(g.get_cov())) == (dx, dP) and g.aux_count() == (0, 0)
    # max_aux_dim reached: 8 of 8 in use, one more scalar is refused, and a NaN below the prior's diagonal is not read
    h8 = g.add_state(np.arange(8.0), np.diag(np.arange(1.0, 9.0)) + np.tril(np.full((8, 8), np.nan), -1))
    x8, P8 = A.digest(g.get_state_vector()[0]), A.digest(g.get_cov())
    with pytest.raises(RuntimeError, match="E_CAPACITY.*max_aux_dim"):
        g.add_state([0.0], [[1.0]])
    with pytest.raises(RuntimeError, match="E_CAPACITY.*max_aux_dim"):
        from_meas()
    assert (A.digest(g.get_state_vector()[0]), A.digest(g.get_cov())) == (x8, P8) and g.aux_count() == (1, 8)
    g.remove_state(h8)
    assert (A.digest(g.get_state_vector()[0]), A.digest(g.get_cov())) == (dx, dP)
    # max_aux_dim = 0 (the default): no room at all; before initialization: E_STATE
    o0 = U.load_options(euroc_yaml, **OVERRIDES)
    g0 = U.VioManager(o0)
    with pytest.raises(RuntimeError, match="E_STATE"):
        g0.add_state([0.0], [[1.0]])
    g0.initialize_with_gt(sim.gt_state(sim.t0))
    P00 = g0.get_cov()
    with pytest.raises(RuntimeError, match="E_CAPACITY.*max_aux_dim = 0"):
        g0.add_state([0.0], [[1.0]])
    assert np.array_equal(g0.get_cov(), P00) and g0.aux_count() == (0, 0)
    g0.close()
    # the handle stays usable
    next_frame()
    h = g.add_state([0.0], [[1.0]])
    g.remove_state(h)


# ---- 7 ----
def test_cpp_facade_adds_reads_fixes_and_removes_on_the_device(tmp_path):
    from test_facade_aux import CFG, build_check, run_env
    exe = build_check(tmp_path)
    r = subprocess.run([exe, CFG, "gpu"], capture_output=True, text=True, timeout=120, env=run_env())
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "AUX applied" in r.stdout and "dead handle: code -1" in r.stdout and "AUX ok" in r.stdout
