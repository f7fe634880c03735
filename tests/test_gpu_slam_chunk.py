"""UpdaterSLAM::update on the device's SLAM-chunk chain (k_feature, the one-launch gate k_chi2_small, k_ekf_MS,
k_ekf_fact, k_ekf_WP, k_chain_apply, the products over k skipping the structurally zero k-steps through the
batch's k-step masks) against the oracle, on the shapes at which the chain takes another path: a single 2-row and a single 4-row feature, a feature whose rows straddle the first 16-row tile
of the stacked batch, a feature with more than 16 rows (the whole batch then takes k_gemm_HPg + k_chi2), one
rejected feature (its rows zeroed by the gate) and a batch in which every feature is rejected (no update).  The
set-up, the yardstick and the bounds are tests/test_gpu_updaters.py::test_updater_level_calls_match_oracle's: the
oracle adopts the device's state before the call; the same used / to_delete flags, state and covariance within
1e-10 relative.  The last test runs the six-launch chain and the seven-launch one (UVIO_HP_SLAM_SEVEN=1) in two
fresh child processes over a small stream with several chunks per frame and compares their digests bit for bit.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_updaters import _feed_imu_until, _same_state, _snapshot_with_candidates, _sync, _used

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Snap:
    pass


@pytest.fixture(scope="module")
def snap(euroc_yaml):
    """Both managers with up to 8 landmarks from UpdaterSLAM::delayed_init, propagated and cloned to the next frame;
    the state there is kept so every case starts from it (set_state on the device manager, the oracle synced)."""
    opts, sim, g, o, window, cands = _snapshot_with_candidates(euroc_yaml, max_slam_features=20, max_slam_in_update=10)
    dset = cands[:8]
    rg, ro = g.slam_delayed_init(dset), o.slam_delayed_init(dset)
    assert _used(rg) == _used(ro)
    _sync(g, o)
    i_next = window[-1] + 1
    t_last, t_next = float(g.get_clone_times()[-1]), float(sim.cam_t[i_next])
    _feed_imu_until(sim, [g, o], t_last, t_next)
    g.propagate_and_clone(t_next)
    o.propagate_and_clone(t_next)
    _same_state(g, o)
    s = _Snap()
    s.opts, s.sim, s.g, s.o, s.t_next = opts, sim, g, o, t_next
    s.times = [float(t) for t in g.get_clone_times()]  # the clone window with the new clone
    s.frame_of = {float(sim.cam_t[i]): i for i in window + [i_next]}
    # landmarks the newest frame sees in both cameras, in the order they were initialized
    s.lms = []
    for (f, _), r in zip(dset, rg):
        if r["used"] and all(f in set(int(x) for x in sim.frames[i_next][k][0]) for k in range(2)):
            s.lms.append(f)
    assert len(s.lms) >= 5, s.lms
    s.state = (g.get_state_vector()[0].copy(), g.get_fej_vector().copy(), g.get_cov().copy())
    yield s
    g.close()


def _meas(s, fid, times, cams=(0, 1), shift=0.0):
    """the landmark's measurements [(cam, t, u, v, un, vn)] at the given times in the given cameras, the raw pixel
    moved by `shift` in u and v (normalized with the oracle's camera model, like every measurement here)"""
    from oracle import oracle as O
    out = []
    for t in times:
        fr = s.sim.frames[s.frame_of[t]]
        for k in cams:
            ids, uv = fr[k]
            j = [int(x) for x in ids].index(fid)
            p = np.array([[uv[j, 0] + shift, uv[j, 1] + shift]], dtype=uv.dtype)
            xy = O.camera_undistort(s.opts.cams[k], p)
            out.append((k, t, float(p[0, 0]), float(p[0, 1]), float(xy[0, 0]), float(xy[0, 1])))
    return out


def _reset(s):
    s.g.set_state(*s.state)
    _sync(s.g, s.o)


def _run(s, feats):
    _reset(s)
    rg, ro = s.g.slam_update(feats), s.o.slam_update(feats)
    assert _used(rg) == _used(ro)
    print("rel diff x %.2e P %.2e" % _same_state(s.g, s.o))
    return rg


def _changed(s):
    return not np.array_equal(s.g.get_cov(), s.state[2])


def test_one_mono_feature(snap):
    """2 rows: one 16-row tile mostly padding, one feature in the batch"""
    rg = _run(snap, [(snap.lms[0], _meas(snap, snap.lms[0], [snap.t_next], cams=(0,)))])
    assert rg[0]["used"] and _changed(snap)


def test_one_stereo_feature(snap):
    """4 rows"""
    rg = _run(snap, [(snap.lms[1], _meas(snap, snap.lms[1], [snap.t_next]))])
    assert rg[0]["used"] and _changed(snap)


def test_feature_across_the_tile_boundary(snap):
    """rows 2, 4, 4, 4, 4: the last feature sits on rows 14 - 17 of the stacked batch, across the first 16-row tile
    boundary of the S tile pairs and of M's column tiles"""
    L = snap.lms
    feats = [(L[0], _meas(snap, L[0], [snap.t_next], cams=(0,)))] + [(f, _meas(snap, f, [snap.t_next])) for f in L[1:5]]
    assert [2 * len(m) for _, m in feats] == [2, 4, 4, 4, 4]
    rg = _run(snap, feats)
    assert sum(r["used"] for r in rg) >= 4 and _changed(snap)


def test_feature_with_more_than_16_rows_takes_the_old_gate(snap):
    """one feature with 5 stereo times (20 rows) in the list: the batch is gated by k_gemm_HPg + k_chi2"""
    def both_cams(f):
        return [t for t in snap.times if t in snap.frame_of and
                all(f in set(int(x) for x in snap.sim.frames[snap.frame_of[t]][k][0]) for k in range(2))]
    big = next(f for f in snap.lms if len(both_cams(f)) >= 5)
    L = [f for f in snap.lms if f != big]
    feats = [(L[0], _meas(snap, L[0], [snap.t_next])), (big, _meas(snap, big, both_cams(big)[-5:])),
             (L[1], _meas(snap, L[1], [snap.t_next], cams=(0,)))]
    assert [2 * len(m) for _, m in feats] == [4, 20, 2]
    rg = _run(snap, feats)
    assert sum(r["used"] for r in rg) >= 2 and _changed(snap)


def test_one_rejected_feature(snap):
    """the second feature's pixels moved by 50 px: the gate rejects it (its rows of H and T zeroed) and the update
    uses the others"""
    L = snap.lms
    feats = [(L[0], _meas(snap, L[0], [snap.t_next])), (L[1], _meas(snap, L[1], [snap.t_next], shift=50.0)),
             (L[2], _meas(snap, L[2], [snap.t_next], cams=(0,))), (L[3], _meas(snap, L[3], [snap.t_next]))]
    rg = _run(snap, feats)
    assert not rg[1]["used"] and sum(r["used"] for r in rg) == 3 and _changed(snap)


def test_all_features_rejected_leaves_the_state_alone(snap):
    """every feature a gross outlier: no update, the state bit-equal to the state before the call"""
    L = snap.lms
    feats = [(f, _meas(snap, f, [snap.t_next], cams=((0,) if k == 0 else (0, 1)), shift=50.0)) for k, f in enumerate(L[:4])]
    rg = _run(snap, feats)
    assert not any(r["used"] for r in rg)
    x, fej, P = snap.state
    assert snap.g.get_state_vector()[0].tobytes() == x.tobytes()
    assert snap.g.get_fej_vector().tobytes() == fej.tobytes()
    assert snap.g.get_cov().tobytes() == P.tobytes()


def test_new_chain_equals_the_seven_launch_chain_bit_for_bit():
    """two fresh child processes over 25 frames with chunks of 4 landmarks (several chunks per frame), with and
    without UVIO_HP_SLAM_SEVEN: equal SHA-256 of the per-frame state vectors and the final covariance"""
    script = os.path.join(ROOT, "tests", "slam_chain_digest.py")
    procs = []
    for seven in (False, True):
        env = dict(os.environ)
        env.pop("UVIO_HP_SLAM_SEVEN", None)
        if seven:
            env["UVIO_HP_SLAM_SEVEN"] = "1"
        procs.append(subprocess.Popen([sys.executable, script, "25"], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE))
    lines = []
    for p in procs:
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, err.decode()[-2000:]
        lines.append(out.decode().strip().splitlines()[-1].split())
    print(lines)
    (_, d_new, _, n_new, _, _), (_, d_old, _, n_old, _, _) = lines
    assert int(n_new) >= 50 and n_new == n_old  # SLAM chunks ran: well over one chunk of 4 per frame on average
    assert d_new == d_old
