"""GPU parity of the landmark representations (LandmarkRepresentation.h:38) through the update chain: the HIP path
against the oracle in lock-step (test_gpu_parity.run_lockstep and _check_lockstep with their bounds unchanged:
1e-9 m triangulation, 1e-11 chi2, 1e-10 state and P, the steering cap, equal accept / reject decisions), for

  feat_rep_msckf  GLOBAL_FULL_INVERSE_DEPTH (1), ANCHORED_FULL_INVERSE_DEPTH (3) and ANCHORED_INVERSE_DEPTH_SINGLE
                  (5, which UpdaterMSCKF linearizes as ANCHORED_MSCKF_INVERSE_DEPTH, UpdaterMSCKF.cpp:181-183)
  feat_rep_slam   1 and 3: (theta, phi, rho) landmarks; 5: the one-dimensional landmark (rho, the bearing beside the
                  state) with its bearing projection; each through the SLAM update, the delayed initialization, the
                  anchor change (reps 3 and 5; a global landmark is never re-anchored) and the updater-level calls

plus uvio_hp_get_features_slam (VioManager::get_features_SLAM) against the oracle's active tracks and a numpy
conversion of the state vector.  The streams are test_gpu_parity's (test_lockstep_msckf_parity /
test_lockstep_slam_parity).
"""
import functools

import numpy as np
import pytest

from conftest import EUROC
from test_gpu_parity import _check_lockstep, _rel, _sim, run_lockstep
from test_gpu_updaters import _feed_imu_until, _frames_at, _same_state, _sync, _tracks, _used

pytestmark = pytest.mark.gpu

SLAM_KW = dict(max_msckf_in_update=100, max_slam_features=20, max_slam_in_update=10, dt_slam_delay=0.3)


def _landmarks(x, meta):
    """[(covariance id, size, value)] of the landmark variables (kind 4) of a state vector: the values of the
    IMU (16 for 15), a pose (7 for 6) and a quaternion (4 for 3) are one longer than their covariance blocks"""
    out, k = [], 0
    for kind, cid, size in meta:
        vlen = size + 1 if kind in (0, 2, 3) else size
        if kind == 4:
            out.append((int(cid), int(size), x[k:k + vlen].copy()))
        k += vlen
    assert k == len(x)
    return out


@pytest.mark.parametrize("rep", [1, 3, 5])
def test_lockstep_msckf_representation(rep):
    import uvio_amd as U
    opts = U.load_options(EUROC, max_msckf_in_update=200, max_slam_features=0, feat_rep_msckf=rep)
    steps = run_lockstep(opts, _sim(opts, 30, spawn=120), 30)
    assert len(steps) == 30
    assert sum(a["timing"]["n_msckf"] for a, _ in steps) > 0
    print("worst", _check_lockstep(steps))


@functools.lru_cache(maxsize=None)
def _slam_run(rep, do_fej=1, mono=False):
    """one lock-step SLAM run per representation, shared by the tests below: per frame also the device's landmark
    points and the oracle's active tracks"""
    import uvio_amd as U
    kw = dict(num_cameras=1, use_stereo=0) if mono else {}
    opts = U.load_options(EUROC, feat_rep_msckf=4, feat_rep_slam=rep, do_fej=do_fej, **SLAM_KW, **kw)

    def extra(g, o, a, b):
        a["slam_pts"] = g.get_features_slam()
        b["active"] = o.get_active_tracks()

    return run_lockstep(opts, _sim(opts, 30, spawn=80, frac_long=0.3), 30, extra=extra)


def _check_slam_run(steps, rep):
    assert len(steps) == 30
    assert sum(a["timing"]["n_slam"] for a, _ in steps) > 0
    assert sum(a["timing"]["n_slam_delayed"] for a, _ in steps) > 0
    nac = sum(a["timing"]["n_anchor_change"] for a, _ in steps)
    assert (nac == 0) if rep == 1 else (nac > 0), nac
    seen = 0
    for a, b in steps:
        assert a["P"].shape == b["P"].shape  # the covariance dimension, on every frame
        assert np.array_equal(a["meta"], b["meta"])
        for _, size, v in _landmarks(a["x"], a["meta"]):
            assert size == len(v) == (1 if rep == 5 else 3)
            seen += 1
    assert seen > 0
    print("worst", _check_lockstep(steps))


@pytest.mark.parametrize("rep", [1, 3, 5])
def test_lockstep_slam_representation(rep):
    _check_slam_run(_slam_run(rep), rep)


def test_lockstep_slam_rep3_without_fej():
    """do_fej off: get_feature_jacobian_representation linearizes at the current anchor pose and the landmark's
    get_xyz(true) feeds only the anchor change's first estimate"""
    _check_slam_run(_slam_run(3, 0), 3)


def test_lockstep_slam_rep5_mono():
    """one camera: frames with a single measurement of a landmark occur all the time, and UpdaterSLAM::update
    needs two for the bearing projection (UpdaterSLAM.cpp:286-295), so that rule decides which landmarks update;
    the landmark counts agree per frame (_check_lockstep)"""
    _check_slam_run(_slam_run(5, 1, True), 5)


@pytest.mark.parametrize("rep", [1, 3, 5])
def test_get_features_slam(rep):
    """every landmark as a global point: equal to the oracle's active-track position of the same id (formed by
    its own retriangulation from its own state, VioManagerHelper.cpp:190-388), and for the global representation
    to the numpy conversion of the state vector; the state bound, 1e-10 relative"""
    steps = _slam_run(rep)
    compared = 0
    for a, b in steps:
        pts = a["slam_pts"]
        lms = _landmarks(a["x"], a["meta"])
        assert len(pts) == len(lms) == a["timing"]["n_slam"]
        _, pos, _ = b["active"]
        for fid, p in pts.items():
            if fid in pos:
                assert _rel(p, pos[fid]) < 1e-10, (fid, p, pos[fid])
                compared += 1
        if rep == 1:
            # dicts keep the insertion order: the landmarks' order in the state vector
            for p, (_, _, v) in zip(pts.values(), lms):
                ref = np.array([np.cos(v[0]) * np.sin(v[1]), np.sin(v[0]) * np.sin(v[1]), np.cos(v[1])]) / v[2]
                assert _rel(p, ref) < 1e-10
    assert compared > 20


@pytest.mark.parametrize("rep", [3, 5])
def test_updater_level_calls_representation(rep):
    """uvio_hp_slam_delayed_init, uvio_hp_slam_update and uvio_hp_slam_change_anchors on a snapshot against the
    oracle's restatement of the same calls (the pattern of test_gpu_updaters.test_updater_level_calls_match_oracle).
    The new landmarks are anchored at the newest clone, so the window is advanced (propagate_and_clone,
    change_anchors, marginalize_old_clone) until that clone is the one to marginalize and the landmarks move."""
    import uvio_amd as U
    from oracle import oracle as O
    from uvio_amd.sim import SimStream
    opts = U.load_options(EUROC, max_msckf_in_update=60, max_slam_features=20, max_slam_in_update=10,
                          dt_slam_delay=100.0, feat_rep_msckf=4, feat_rep_slam=rep)
    n = 14
    sim = SimStream(opts, duration=(n + opts.max_clone_size + 6) / opts.track_frequency + 1.2, seed=11, spawn=40,
                    frac_long=0.5)
    g, o = U.VioManager(opts), O.OracleManager(opts)
    sim.run([g, o], n_frames=n, before_frame=lambda nf, t: _sync(g, o))
    _sync(g, o)
    ct = g.get_clone_times()
    window = _frames_at(sim, ct)
    t_last, i_next = float(ct[-1]), window[-1] + 1
    tracks = _tracks(sim, opts, window)
    nxt = set(int(f) for k in range(sim.K) for f in sim.frames[i_next][k][0])
    longf = sorted(f for f, m in tracks.items() if len(set(x[1] for x in m)) >= 6)
    dset = [(f, tracks[f]) for f in longf if f in nxt][:8]
    assert len(dset) >= 4

    N0 = g.cov_dim()
    rg, ro = g.slam_delayed_init(dset), o.slam_delayed_init(dset)
    assert _used(rg) == _used(ro)
    nlm = sum(r["used"] for r in rg)
    assert nlm >= 2 and g.cov_dim() == N0 + (1 if rep == 5 else 3) * nlm
    _same_state(g, o)

    moved = 0
    for k in range(opts.max_clone_size):
        _sync(g, o)
        t_next = float(sim.cam_t[i_next + k])
        _feed_imu_until(sim, [g, o], t_last, t_next)
        g.propagate_and_clone(t_next)
        o.propagate_and_clone(t_next)
        t_last = t_next
        _same_state(g, o)
        if k == 0:  # UpdaterSLAM::update with the landmarks' tracks including the new frame
            _sync(g, o)
            tracks2 = _tracks(sim, opts, window + [i_next])
            lms = [(f, tracks2[f]) for (f, _), r in zip(dset, rg) if r["used"]]
            rg2, ro2 = g.slam_update(lms), o.slam_update(lms)
            assert _used(rg2) == _used(ro2)
            assert sum(r["used"] for r in rg2) >= 1
            _same_state(g, o)
        _sync(g, o)
        before = [v for _, _, v in _landmarks(*g.get_state_vector())]
        pts = g.get_features_slam()
        g.slam_change_anchors()
        o.slam_change_anchors()
        _same_state(g, o)
        after = [v for _, _, v in _landmarks(*g.get_state_vector())]
        changed = sum(not np.array_equal(x, y) for x, y in zip(before, after))
        if changed:  # re-anchored: the same global points through the new anchor
            moved += changed
            pts2 = g.get_features_slam()
            assert list(pts) == list(pts2)
            for fid in pts:
                assert _rel(pts2[fid], pts[fid]) < 1e-10
        _sync(g, o)
        g.marginalize_old_clone()
        o.marginalize_old_clone()
        _same_state(g, o)
    assert moved >= nlm
    g.close()

