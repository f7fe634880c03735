"""GPU parity of the Updater-level C ABI (include/uvio_hp.h "Updater-level boundary"):
uvio_hp_msckf_update / slam_delayed_init / slam_update / slam_change_anchors / marginalize_* /
propagate_and_clone / uwb_update_single called with caller-built features on a state snapshot, against
the oracle's restatement of the reference's own calls (UpdaterMSCKF::update, UpdaterSLAM::delayed_init /
update / change_anchors, StateHelper::marginalize_*, Propagator::propagate_and_clone,
UpdaterUWB::update_single) on the same snapshot and features.

The snapshot comes from a lock-step run of both managers over the simulated stream (so both hold the same
variables); features are the stream's TrackSIM measurements over the clone times, normalized with the
oracle's camera model.  Before each call the oracle adopts the device's state, so every call is compared
on identical inputs.  Tolerances as in test_gpu_parity.py's lock-step frames: the same features used /
erased / flagged to_delete, the same state layout, state and covariance within 1e-10 relative.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def _sync(g, o):
    o.set_state(g.get_state_vector()[0], g.get_fej_vector(), g.get_cov())


def _same_state(g, o, tol=1e-10):
    xg, mg = g.get_state_vector()
    xo, mo = o.get_state_vector()
    assert np.array_equal(mg, mo), "state layouts differ"
    Pg, Po = g.get_cov(), o.get_cov()
    assert _rel(xg, xo) < tol, _rel(xg, xo)
    assert _rel(Pg, Po) < tol, _rel(Pg, Po)
    return _rel(xg, xo), _rel(Pg, Po)


def _tracks(sim, opts, frames):
    """featid -> [(cam, t, u, v, un, vn)] over the given sim frame indices, in observation order"""
    from oracle import oracle as O
    tr = {}
    for i in frames:
        t = float(sim.cam_t[i])
        for k, (ids, uv) in enumerate(sim.frames[i]):
            if len(ids) == 0:
                continue
            xy = O.camera_undistort(opts.cams[k], uv)
            for j, fid in enumerate(ids):
                tr.setdefault(int(fid), []).append((k, t, float(uv[j, 0]), float(uv[j, 1]), float(xy[j, 0]),
                                                    float(xy[j, 1])))
    return tr


def _frames_at(sim, times):
    idx = []
    for t in times:
        k = int(np.argmin(np.abs(sim.cam_t - t)))
        assert abs(sim.cam_t[k] - t) < 1e-9
        idx.append(k)
    return idx


def _feed_imu_until(sim, mgrs, t_from, t_to):
    lag = 1.0 / sim.imu_rate + 1e-9
    for i, t in enumerate(sim.imu_t):
        if t_from + lag <= t < t_to + lag:
            for m in mgrs:
                m.feed_measurement_imu(t, sim.wm[i], sim.am[i])


def _used(res):
    return [(r["featid"], r["used"], r["to_delete"]) for r in res]


def test_updater_level_calls_match_oracle(euroc_yaml):
    import uvio_amd as U
    from oracle import oracle as O
    from uvio_amd.sim import SimStream
    opts = U.load_options(euroc_yaml, max_msckf_in_update=60, max_slam_features=20, max_slam_in_update=10,
                          dt_slam_delay=100.0)  # no SLAM inside the frames: the landmarks come from the calls below
    n = 14
    sim = SimStream(opts, duration=(n + 6) / opts.track_frequency + 1.2, seed=11, spawn=40, frac_long=0.5)
    g, o = U.VioManager(opts), O.OracleManager(opts)
    sim.run([g, o], n_frames=n, before_frame=lambda nf, t: _sync(g, o))
    _sync(g, o)
    ct = g.get_clone_times()
    assert len(ct) == opts.max_clone_size and np.allclose(ct, o.get_clone_times())
    window = _frames_at(sim, ct)
    t_last, i_next = float(ct[-1]), window[-1] + 1
    tracks = _tracks(sim, opts, window)
    nxt = set(int(f) for k in range(sim.K) for f in sim.frames[i_next][k][0])
    longf = sorted(f for f, m in tracks.items() if len(set(x[1] for x in m)) >= 6)
    # delayed-init candidates: long tracks that continue into the next frame; MSCKF: the other long ones
    dset = [(f, tracks[f]) for f in longf if f in nxt][:8]
    mset = [(f, tracks[f]) for f in longf if f not in dict(dset)][:40]
    short = [(10 ** 9 + k, tracks[f][:1]) for k, f in enumerate(longf[:2])]  # one measurement: too few
    assert len(dset) >= 4 and len(mset) >= 20

    # UpdaterMSCKF::update
    rg, ro = g.msckf_update(mset + short), o.msckf_update(mset + short)
    assert _used(rg) == _used(ro)
    assert sum(r["used"] for r in rg) >= 10
    assert all(r["status"] == 1 for r in rg[-len(short):])
    _same_state(g, o)

    # UpdaterSLAM::delayed_init: accepted features become landmarks (3 more covariance columns each)
    _sync(g, o)
    N0 = g.cov_dim()
    rg, ro = g.slam_delayed_init(dset), o.slam_delayed_init(dset)
    assert _used(rg) == _used(ro)
    nlm = sum(r["used"] for r in rg)
    assert nlm >= 2 and g.cov_dim() == N0 + 3 * nlm
    _same_state(g, o)

    # Propagator::propagate_and_clone to the next frame
    _sync(g, o)
    t_next = float(sim.cam_t[i_next])
    _feed_imu_until(sim, [g, o], t_last, t_next)
    g.propagate_and_clone(t_next)
    o.propagate_and_clone(t_next)
    assert g.get_clone_times()[-1] == t_next
    _same_state(g, o)

    # UpdaterSLAM::update with the landmarks' tracks including the new frame
    _sync(g, o)
    tracks2 = _tracks(sim, opts, window + [i_next])
    lms = [(f, tracks2[f]) for (f, _), r in zip(dset, rg) if r["used"]]
    rg2, ro2 = g.slam_update(lms), o.slam_update(lms)
    assert _used(rg2) == _used(ro2)
    assert sum(r["used"] for r in rg2) >= 1
    _same_state(g, o)

    # UpdaterSLAM::change_anchors, StateHelper::marginalize_slam / marginalize_old_clone
    for step in ("slam_change_anchors", "marginalize_slam", "marginalize_old_clone"):
        _sync(g, o)
        getattr(g, step)()
        getattr(o, step)()
        _same_state(g, o)
    assert len(g.get_clone_times()) == opts.max_clone_size
    g.close()


def test_updater_level_rejects_unknown_slam_landmark(euroc_yaml):
    import uvio_amd as U
    from uvio_amd.sim import SimStream
    opts = U.load_options(euroc_yaml, max_msckf_in_update=60, max_slam_features=0)
    sim = SimStream(opts, duration=8 / opts.track_frequency + 1.2, seed=3, spawn=30)
    g = U.VioManager(opts)
    sim.run(g, n_frames=6)
    t = float(g.get_clone_times()[-1])
    with pytest.raises(RuntimeError, match="E_ARG"):
        g.slam_update([(987654321, [(0, t, 100.0, 100.0, 0.1, 0.1)])])
    with pytest.raises(RuntimeError, match="E_ARG"):
        g.msckf_update([(1, [(7, t, 100.0, 100.0, 0.1, 0.1)])])  # camera id out of range
    g.close()


def test_updater_level_error_names_the_reference_routine(euroc_yaml):
    """A failed updater-level call names the reference routine it stands for (UpdaterSLAM::delayed_init here), not
    the device chain that runs it.  The error is an ordinary capacity refusal, raised before any device work:
    200 candidates would need 600 more covariance columns than the state's capacity has."""
    import uvio_amd as U
    from uvio_amd.sim import SimStream
    opts = U.load_options(euroc_yaml, max_msckf_in_update=60, max_slam_features=0)
    sim = SimStream(opts, duration=8 / opts.track_frequency + 1.2, seed=3, spawn=30)
    g = U.VioManager(opts)
    sim.run(g, n_frames=6)
    ct = g.get_clone_times()
    N0 = g.cov_dim()
    two = [(0, float(ct[-2]), 100.0, 100.0, 0.1, 0.1), (0, float(ct[-1]), 101.0, 100.0, 0.11, 0.1)]
    with pytest.raises(RuntimeError, match=r"E_CAPACITY.*UpdaterSLAM::delayed_init"):
        g.slam_delayed_init([(10 ** 9 + k, two) for k in range(200)])
    assert g.cov_dim() == N0  # refused whole: nothing was initialized
    with pytest.raises(RuntimeError, match=r"E_ARG.*UpdaterSLAM::update"):
        g.slam_update([(987654321, two)])
    g.close()


def _snapshot_with_candidates(euroc_yaml, **kw):
    """test_updater_level_calls_match_oracle's fixture: both managers in lock-step over 14 frames, the oracle
    synced; returns them with the stream, the clone window's frame indices and the delayed-init candidates (long
    tracks that continue into the next frame), all that are available."""
    import uvio_amd as U
    from oracle import oracle as O
    from uvio_amd.sim import SimStream
    opts = U.load_options(euroc_yaml, max_msckf_in_update=60, dt_slam_delay=100.0, **kw)
    n = 14
    sim = SimStream(opts, duration=(n + 6) / opts.track_frequency + 1.2, seed=11, spawn=40, frac_long=0.5)
    g, o = U.VioManager(opts), O.OracleManager(opts)
    sim.run([g, o], n_frames=n, before_frame=lambda nf, t: _sync(g, o))
    _sync(g, o)
    ct = g.get_clone_times()
    assert len(ct) == opts.max_clone_size and np.allclose(ct, o.get_clone_times())
    window = _frames_at(sim, ct)
    tracks = _tracks(sim, opts, window)
    nxt = set(int(f) for k in range(sim.K) for f in sim.frames[window[-1] + 1][k][0])
    longf = sorted(f for f, m in tracks.items() if len(set(x[1] for x in m)) >= 6)
    cands = [(f, tracks[f]) for f in longf if f in nxt]
    return opts, sim, g, o, window, cands


def test_delayed_init_beyond_the_configured_landmark_count(euroc_yaml):
    """UpdaterSLAM::delayed_init takes whatever list it is given: 8 candidates with max_slam_features = 2.  The
    update chain's regions used to be sized from max_slam_features (6 for this config); the covariance has room
    for all 8 (its capacity includes spare clone and anchor columns), so the call must initialize them as the
    oracle does."""
    opts, sim, g, o, window, cands = _snapshot_with_candidates(euroc_yaml, max_slam_features=2, max_slam_in_update=10)
    dset = cands[:8]
    assert len(dset) == 8
    N0 = g.cov_dim()
    rg, ro = g.slam_delayed_init(dset), o.slam_delayed_init(dset)
    assert _used(rg) == _used(ro)
    used = sum(r["used"] for r in rg)
    print("delayed init: %d of %d used, N %d -> %d" % (used, len(dset), N0, g.cov_dim()))
    assert used >= 7
    assert g.cov_dim() == N0 + 3 * used == o.get_cov().shape[0]
    print("rel diff x %.2e P %.2e" % _same_state(g, o))
    g.close()


def _stereo_cut(meas, which):
    """the track's measurements at the stereo times (clone times at which both cameras saw it, ascending) with the
    indices `which`: two measurements per time"""
    times = sorted(set(m[1] for m in meas))
    both = [t for t in times if len(set(m[0] for m in meas if m[1] == t)) == 2]
    keep = set(both[i] for i in which) if both else set()
    return [m for m in meas if m[1] in keep]


@pytest.mark.parametrize("rep,d", [(4, 3), (5, 1)])
def test_delayed_init_smallest_candidates(euroc_yaml, rep, d):
    """The smallest candidates UpdaterSLAM::delayed_init can hand the update chain, in one call: a candidate of
    exactly two measurements (both cameras at its last stereo clone time: 2 m - 3 = 1 update row beside the d
    initializing rows), one of two stereo times (4 measurements, 5 update rows) and one full-length track, at
    d = 3 (ANCHORED_MSCKF_INVERSE_DEPTH) and d = 1 (ANCHORED_INVERSE_DEPTH_SINGLE).

    The short candidates are chosen with the oracle alone: a second oracle over the same stream adopts the
    snapshot and takes the truncated candidates one at a time; the first one it initializes is used (most
    two-measurement cuts fail the triangulation's baseline checks, and a rejected one leaves the oracle as it
    was).  The one-row candidate goes first in the list, so the call sees it at the state it was probed at, and
    the oracle must accept it there: the test cannot pass on rejected candidates alone.  Both representations have
    such a candidate in this snapshot (the 29th of 289 at either d)."""
    from oracle import oracle as O
    opts, sim, g, o, window, cands = _snapshot_with_candidates(euroc_yaml, max_slam_features=20, max_slam_in_update=10,
                                                               feat_rep_slam=rep)

    def first_accepted(which, skip=()):
        probe = O.OracleManager(opts)
        sim.run([probe], n_frames=14)
        for f, meas in cands:
            short = _stereo_cut(meas, which)
            if f in skip or len(short) != 2 * len(which):
                continue
            _sync(g, probe)
            if probe.slam_delayed_init([(f, short)])[0]["used"]:
                return f, short
        return None

    one_row = first_accepted([-1])
    assert one_row is not None, "no two-measurement candidate passes the oracle"
    five_rows = first_accepted([0, -1], skip=(one_row[0],))
    assert five_rows is not None, "no two-stereo-time candidate passes the oracle"
    full = next(c for c in cands if c[0] not in (one_row[0], five_rows[0]))
    dset = [one_row, five_rows, full]
    assert [len(m) for _, m in dset[:2]] == [2, 4] and len(full[1]) >= 12
    assert len(set(m[1] for m in one_row[1])) == 1 and len(set(m[1] for m in five_rows[1])) == 2

    _sync(g, o)
    N0 = g.cov_dim()
    rg, ro = g.slam_delayed_init(dset), o.slam_delayed_init(dset)
    print("rep %d: used (device, oracle) %s" % (rep, [(a["used"], b["used"]) for a, b in zip(rg, ro)]))
    assert ro[0]["used"], "the oracle rejected the one-row candidate it accepted alone"
    assert _used(rg) == _used(ro)
    used = sum(r["used"] for r in rg)
    assert g.cov_dim() == N0 + d * used == o.get_cov().shape[0]
    print("rel diff x %.2e P %.2e" % _same_state(g, o))
    g.close()


def test_slam_update_takes_its_list_as_one_batch(euroc_yaml):
    """UpdaterSLAM::update linearizes its whole list at one state and applies one EKF update; the chunks of
    max_slam_in_update are VioManager's.  With max_slam_in_update = 2 and 8 landmarks in one call, chunking
    would differ from the oracle's single batch by 2e-5 in x and 6e-4 in P on this input."""
    opts, sim, g, o, window, cands = _snapshot_with_candidates(euroc_yaml, max_slam_features=20, max_slam_in_update=2)
    dset = cands[:8]
    rg, ro = g.slam_delayed_init(dset), o.slam_delayed_init(dset)
    assert _used(rg) == _used(ro)
    _same_state(g, o)
    _sync(g, o)
    i_next = window[-1] + 1
    t_last, t_next = float(g.get_clone_times()[-1]), float(sim.cam_t[i_next])
    _feed_imu_until(sim, [g, o], t_last, t_next)
    g.propagate_and_clone(t_next)
    o.propagate_and_clone(t_next)
    _same_state(g, o)
    _sync(g, o)
    tracks2 = _tracks(sim, opts, window + [i_next])
    lms = [(f, tracks2[f]) for (f, _), r in zip(dset, rg) if r["used"]]
    rg2, ro2 = g.slam_update(lms), o.slam_update(lms)
    assert _used(rg2) == _used(ro2)
    used = sum(r["used"] for r in rg2)
    print("slam update: %d of %d landmarks used" % (used, len(lms)))
    assert used >= 5  # more than two chunks' worth
    print("rel diff x %.2e P %.2e" % _same_state(g, o))
    g.close()


def test_uwb_update_single_matches_oracle(euroc_yaml):
    """UpdaterUWB::update_single (UpdaterUWB.cpp:53-90) through the C ABI on a state snapshot, fixed and
    estimated anchors, one range consistent with the ground truth and one 20 m off (chi2-gated on both)."""
    import uvio_amd as U
    from uvio_amd import _native as N
    from oracle import oracle as O
    from uvio_amd.sim import SimStream
    from test_gpu_parity import make_anchors
    opts = U.load_options(euroc_yaml, max_msckf_in_update=60, max_slam_features=0, use_uwb=1,
                          do_calib_uwb_extrinsics=1, min_dist_to_use_uwb=0.05)
    for k, v in enumerate([0.05, -0.02, 0.03]):
        opts.p_IinU[k] = v
    anchors = make_anchors(N)
    n = 10
    sim = SimStream(opts, duration=(n + 2) / opts.track_frequency + 1.2, seed=4, spawn=40, anchors=anchors,
                    uwb_rate=10.0, uwb_sigma=0.1)
    g, o = U.VioManager(opts), O.OracleManager(opts)
    sim.run([g, o], n_frames=n, before_frame=lambda nf, t: _sync(g, o),
            after_init=lambda m: m.try_to_initialize_uwb_anchors(anchors))
    t, _ = g.get_imu_state()
    p_U = sim.traj.R_ItoG(t) @ (-np.array(opts.p_IinU[:])) + sim.traj.pos(t)
    applied, gated = 0, 0
    for a in anchors:
        true = (1 + a.dist_bias) * np.linalg.norm(np.array(a.p_AinG[:]) - p_U) + a.const_bias
        for rng in (true + 0.05, true + 20.0):
            _sync(g, o)
            ag = g.uwb_update_single(t, a.id, rng)
            ao = o.uwb_update_single(t, a.id, rng)
            assert ag == ao
            applied += ag
            gated += not ag
            _same_state(g, o)
    assert applied >= 3 and gated >= 3
    g.close()


def test_fatal_error_stops_the_handle(euroc_yaml):
    """A negative covariance diagonal after an update is fatal in the reference (StateHelper.cpp:171-182,
    std::exit): the call returns UVIO_HP_E_NUMERIC and every later state-changing call UVIO_HP_E_STATE naming it,
    while the getters still read the state."""
    import uvio_amd as U
    from uvio_amd import _native as N
    from uvio_amd.sim import SimStream
    from test_gpu_parity import make_anchors
    opts = U.load_options(euroc_yaml, max_msckf_in_update=60, max_slam_features=0, use_uwb=1,
                          do_calib_uwb_extrinsics=1, min_dist_to_use_uwb=0.05)
    anchors = make_anchors(N)
    n = 8
    sim = SimStream(opts, duration=(n + 2) / opts.track_frequency + 1.2, seed=4, spawn=40, anchors=anchors,
                    uwb_rate=10.0, uwb_sigma=0.1)
    g = U.VioManager(opts)
    sim.run(g, n_frames=n, after_init=lambda m: m.try_to_initialize_uwb_anchors(anchors))
    x, _ = g.get_state_vector()
    P = g.get_cov()
    P[-1, -1] = -1.0  # the last variable (outside the range's columns) gets a negative variance
    g.set_state(x, g.get_fej_vector(), P)
    t, _ = g.get_imu_state()
    a = anchors[-1]
    p_U = sim.traj.R_ItoG(t) @ (-np.array(opts.p_IinU[:])) + sim.traj.pos(t)
    rng = (1 + a.dist_bias) * np.linalg.norm(np.array(a.p_AinG[:]) - p_U) + a.const_bias
    with pytest.raises(RuntimeError, match="E_NUMERIC"):
        g.uwb_update_single(t, a.id, rng)
    with pytest.raises(RuntimeError, match="E_STATE.*stopped"):
        g.uwb_update_single(t, a.id, rng)
    with pytest.raises(RuntimeError, match="E_STATE"):
        g.propagate_and_clone(t + 0.05)
    assert g.get_cov().shape == P.shape and np.all(np.isfinite(g.get_state_vector()[0]))
    g.close()
