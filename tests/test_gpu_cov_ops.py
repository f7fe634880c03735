"""The covariance bookkeeping kernels on the device (uvio_amd/csrc/kernels_cov.hip: k_prop_T, k_prop_write, the fused
k_prop_clone, k_clone, k_marginalize, k_marginalize_multi, k_compact, k_marginal_gather) through their standalone
twins uvio_hp_debug_cov_propagate_p / uvio_hp_debug_cov_gather_p, at the dispatch edges of
Engine::cov_propagate_clone (prop_clone_fits in kernels.h: p <= 32, q <= 32, N p <= 8192).

1. Propagation and clone.  The whole returned buffer -- padding included, pre-filled with a NaN that carries a payload
   -- has the bits of the float64 replay (tests/cov_ref.py: the kernels' summation order, every product and sum
   rounded by itself; the library is built with -ffp-contract=off).  Wherever the fused kernel takes a shape, the forced
   three-kernel path and the fused one return the same bits, and selector 0 reports the path the rule gives.  P is
   asymmetric by a few ulp below the diagonal and Q is NaN below it, so the triangle a kernel reads shows.
2. The gathers, on P[i][j] = 4096 i + j (equality names the source element): k_marginalize and k_marginalize_multi equal
   the sequence of StateHelper::marginalize calls, k_compact equals P[src][:, src] and differs from the multi kernel
   exactly where its flip rule says (so marginalize_slots may use it only on an exactly symmetric P), k_marginal_gather
   takes repeats and any order.  Output columns >= Nn keep their bytes.
3. On a handle: lock-step against the oracle with a 30 x 30 Phi (IMU intrinsics without g-sensitivity, both IMU
   models), the only configuration that enters k_prop_clone with four a0 rounds; and propagate_and_clone +
   marginalize_old_clone with and without the camera time offset, per entry in correlation units.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cov_ref as R  # noqa: E402
import ekf_ref as E  # noqa: E402

pytestmark = pytest.mark.gpu

AUTO, SPLIT, FUSED = 0, 1, 2
DNC = np.array([0.3, -0.02, 1e-3, -1.5, 0.25, 4.0])


def _inputs(N, s0, p, q, seed=0):
    new = np.arange(s0, s0 + p)
    iold = R.iold_case(N, s0, p, q, 5 + seed)
    return R.cov_case(N, 11 + N + seed), new, iold, R.phi_case(new, iold, 17 + seed), R.q_case(p, 23 + seed)


def _run_all_paths(P, s0, new, iold, Phi, Q, want_path, rows=None, clone_src=None, dt_id=-1, ld=None):
    """selector 0, 1 and (where the fused kernel takes the shape) 2: each buffer has the replay's bits, the path that
    ran is the stated one; returns the number of device calls"""
    import uvio_amd as U
    dnc = DNC if dt_id >= 0 else None
    want = R.expected_buffer(P, new, iold, Phi, Q, clone_src, dt_id, dnc, ld=ld)
    paths = [(AUTO, want_path), (SPLIT, SPLIT)] + ([(FUSED, FUSED)] if want_path == FUSED else [])
    for path, ran_want in paths:
        buf, ran = U.cov_propagate_p(P, s0, iold, Phi, Q, rows=rows, clone_src=clone_src, dt_id=dt_id, dnc=dnc, path=path,
                                     ld=ld, fill=R.NAN_FILL)
        assert ran == ran_want, (path, ran, ran_want)
        if not R.same_bits(buf, want):
            bad = np.argwhere(buf.view(np.uint64) != want.view(np.uint64))
            i, j = bad[0]
            raise AssertionError("path %d: %d entries differ from the replay, first (%d, %d): %r != %r"
                                 % (path, len(bad), i, j, buf[i, j], want[i, j]))
    if want_path == SPLIT and clone_src is not None:
        with pytest.raises(RuntimeError, match="E_CAPACITY"):
            U.cov_propagate_p(P, s0, iold, Phi, Q, clone_src=clone_src, dt_id=dt_id, dnc=dnc, path=FUSED, ld=ld)
    return len(paths)


# ---- 1 ----
# (N, p, extra ld, the path selector 0 takes): the i += blockDim.x loops' second trip (N > 512), N p = 8190 / 8205 at
# p = 15, 8190 / 8220 at p = 30, 8192 / 8224 at p = 32, p past 32
CLONE_SHAPES = [(15, 15, 5, FUSED), (16, 15, 0, FUSED), (511, 15, 5, FUSED), (512, 15, 5, FUSED), (513, 15, 5, FUSED),
                (546, 15, 5, FUSED), (547, 15, 5, SPLIT), (273, 30, 5, FUSED), (274, 30, 5, SPLIT),
                (256, 32, 5, FUSED), (257, 32, 5, SPLIT), (100, 33, 5, SPLIT), (120, 39, 5, SPLIT)]


@pytest.mark.parametrize("N,p,pad,want_path", CLONE_SHAPES, ids=lambda v: str(v))
def test_propagate_and_clone_at_the_fused_kernels_edges(N, p, pad, want_path):
    P, new, iold, Phi, Q = _inputs(N, 0, p, p)
    dt_id = N - 1 if N > p else -1  # the time-offset column behind the block where there is one
    _run_all_paths(P, 0, new, iold, Phi, Q, want_path, clone_src=0, dt_id=dt_id, ld=N + 6 + pad)


@pytest.mark.parametrize("p,q", [(1, 1), (7, 7), (8, 8), (9, 9), (9, 17), (17, 9)], ids=lambda v: str(v))
def test_partial_groups_of_eight_outputs(p, q):
    """the a0 += 8 rounds of k_prop_clone with a partial last group and the clamped min(a0 + u, p - 1), the block at the
    start, in the middle and at the end of the state, iold the block plus or minus other columns"""
    N = 64
    for s0 in (0, 20, N - p):
        P, new, iold, Phi, Q = _inputs(N, s0, p, q, seed=s0)
        _run_all_paths(P, s0, new, iold, Phi, Q, FUSED, clone_src=min(s0, N - 6), dt_id=(s0 + p) % N, ld=N + 11)


@pytest.mark.parametrize("N,p,want_path", [(64, 15, FUSED), (120, 39, SPLIT)], ids=["fused", "split"])
@pytest.mark.parametrize("dt", ["off", "before", "after"])
def test_time_offset_term_on_both_paths(N, p, want_path, dt):
    s0 = 8
    P, new, iold, Phi, Q = _inputs(N, s0, p, p, seed=3)
    dt_id = {"off": -1, "before": 2, "after": s0 + p + 4}[dt]
    _run_all_paths(P, s0, new, iold, Phi, Q, want_path, clone_src=s0, dt_id=dt_id, ld=N + 11)
    if dt == "off":  # a copy: the clone block is the pose block entry for entry, asymmetry included
        import uvio_amd as U
        buf, _ = U.cov_propagate_p(P, s0, iold, Phi, Q, clone_src=s0, ld=N + 6)
        assert R.same_bits(buf[N:, N:N + 6], buf[s0:s0 + 6, s0:s0 + 6])
        assert R.same_bits(buf[:N, N:N + 6], buf[:N, s0:s0 + 6]) and R.same_bits(buf[N:, :N], buf[s0:s0 + 6, :N])
        assert not np.array_equal(buf[s0:s0 + p, s0:s0 + p], buf[s0:s0 + p, s0:s0 + p].T)  # the block: up to rounding


def test_zupt_bias_walk_without_a_clone():
    """UpdaterZeroVelocity's propagation of the biases: p = q = 6 at s0 = 9, Phi = I, no clone: always the two launches"""
    N = 33
    P, new, iold, _, Q = _inputs(N, 9, 6, 6)
    Phi = np.eye(6)
    _run_all_paths(P, 9, new, iold, Phi, Q, SPLIT, ld=N + 4)
    import uvio_amd as U
    buf, ran = U.cov_propagate_p(P, 9, iold, Phi, Q, ld=N)
    assert ran == SPLIT and np.array_equal(buf[9:15, 9:15], P[9:15, 9:15] + R.sym_upper(Q))
    with pytest.raises(RuntimeError, match="E_ARG"):
        U.cov_propagate_p(P, 9, iold, Phi, Q, path=FUSED)


def test_capacity_limits():
    import uvio_amd as U
    N = 300
    P, new, iold, Phi, Q = _inputs(N, 100, 64, 256)
    _run_all_paths(P, 100, new, iold, Phi, Q, SPLIT, ld=N + 3)
    _run_all_paths(P, 100, new, iold, Phi, Q, SPLIT, clone_src=100, dt_id=7, ld=N + 9)
    for p, q in ((65, 8), (8, 257)):
        with pytest.raises(RuntimeError, match="E_CAPACITY"):
            U.cov_propagate_p(P, 0, np.arange(q), np.zeros((p, q)), np.zeros((p, p)))


@pytest.mark.parametrize("N", [40, 257])
@pytest.mark.parametrize("zero_q", [False, True], ids=["Q", "Q0"])
def test_rows_form_with_a_block_row_phi(N, zero_q):
    """change_anchors' call: variables of sizes 3, 1, 6 at non-adjacent positions, each row of Phi reading its own
    variable's columns and one shared column"""
    from test_cov_ref import _rows_case
    P, rows, iold, Phi, Q = _rows_case(N, zero_q=zero_q)
    _run_all_paths(P, 0, rows, iold, Phi, Q, SPLIT, rows=rows, ld=N + 5)


# ---- 2 ----
def _gather(P, op, ld, **kw):
    import uvio_amd as U
    return U.cov_gather_p(P, op, ld=ld, fill=R.NAN_FILL, **kw)


def _padded(want, ld):
    buf = np.full((want.shape[0], ld), R.NAN_FILL)
    buf[:, :want.shape[1]] = want
    return buf


# N = 135 at the listed blocks; then Nn = N - ms across the 128-column launch edge and past two of them
@pytest.mark.parametrize("N,m0,ms", [(135, 0, 6), (135, 132, 3), (135, 64, 1), (135, 127, 6), (135, 0, 135),
                                     (133, 64, 6), (134, 64, 6), (135, 64, 6), (263, 64, 6)], ids=lambda v: str(v))
def test_single_marginalize(N, m0, ms):
    from uvio_amd import _native as Nt
    P = R.coded(N)
    got = _gather(P, Nt.COV_MARGINALIZE, N + 3, m0=m0, ms=ms)
    assert R.same_bits(got, _padded(R.marginalize_one(P, m0, ms), N + 3))


def _variable_sets(N):
    """2 to 5 removed variables of sizes 1, 3, 6: with an adjacent pair, the first and the last variable"""
    return [[(10, 6), (N - 3, 3)], [(6, 3), (9, 1), (40, 6)], [(0, 6), (6, 3), (70, 1), (N - 6, 6)],
            [(0, 1), (20, 6), (26, 6), (64, 3), (N - 1, 1)]]


@pytest.mark.parametrize("k", range(4))
def test_multi_marginalize_equals_the_sequence_and_compact_the_plain_gather(k):
    from uvio_amd import _native as Nt
    N = 135
    variables = _variable_sets(N)[k]
    src = R.kept_indices(N, variables)
    P, Ps = R.coded(N), R.coded(N, symmetric=True)
    want = R.marginalize_seq(P, variables)
    multi = _gather(P, Nt.COV_MARGINALIZE_MULTI, N + 3, idx=src)
    assert R.same_bits(multi, _padded(want, N + 3))
    compact = _gather(P, Nt.COV_COMPACT, N + 3, idx=src)
    assert R.same_bits(compact, _padded(P[np.ix_(src, src)], N + 3))
    # the precondition marginalize_slots relies on: equal on an exactly symmetric P, and on the asymmetric one
    # different exactly at the entries the flip rule names
    n = src.size
    assert np.array_equal(compact[:, :n] != multi[:, :n], R.flip_mask(src)) and R.flip_mask(src).any()
    assert R.same_bits(_gather(Ps, Nt.COV_COMPACT, N + 3, idx=src), _gather(Ps, Nt.COV_MARGINALIZE_MULTI, N + 3, idx=src))


@pytest.mark.parametrize("Nn", [127, 128, 129, 257])
def test_multi_marginalize_and_compact_across_the_launch_edge(Nn):
    from uvio_amd import _native as Nt
    variables = [(3, 1), (50, 6), (56, 3)]
    N = Nn + 10
    src = R.kept_indices(N, variables)
    assert src.size == Nn
    P = R.coded(N)
    assert R.same_bits(_gather(P, Nt.COV_MARGINALIZE_MULTI, N + 3, idx=src), _padded(R.marginalize_seq(P, variables), N + 3))
    assert R.same_bits(_gather(P, Nt.COV_COMPACT, N + 3, idx=src), _padded(P[np.ix_(src, src)], N + 3))


@pytest.mark.parametrize("m", [1, 3, 63, 64, 65, 130])
def test_marginal_gather_takes_repeats_and_any_order(m):
    from uvio_amd import _native as Nt
    N = 135
    P = R.coded(N)
    rng = np.random.default_rng(m)
    for idx in (np.arange(N - 1, N - 1 - m, -1), rng.integers(0, N, m), np.full(m, 77)):
        idx = idx.astype(np.int32)
        got = _gather(P, Nt.COV_MARGINAL_GATHER, N + 3, idx=idx)
        assert got.shape == (m, m) and np.array_equal(got, P[np.ix_(idx, idx)])


# ---- 3 ----
def _selector0(N, p):
    """what Engine::cov_propagate_clone would do for (N, p, p): the twin's selector 0 on an identity propagation"""
    import uvio_amd as U
    buf, ran = U.cov_propagate_p(np.eye(N), 0, np.arange(p), np.eye(p), np.zeros((p, p)), clone_src=0)
    assert np.array_equal(buf[:N, :N], np.eye(N))
    return ran


@pytest.mark.parametrize("imu_model", [0, 1], ids=["kalibr", "rpng"])
def test_lockstep_phi_30_without_g_sensitivity(imu_model):
    """IMU intrinsics without g-sensitivity: Phi is 30 x 30 (IMU 15, Dw 6, Da 6, and R_ACCtoIMU for the kalibr model
    or R_GYROtoIMU for the rpng one), the frame's propagation runs in k_prop_clone"""
    import uvio_amd as U
    from test_gpu_configs import _cfg, _lockstep
    from test_gpu_parity import _check_lockstep
    opts = U.load_options(_cfg("rpng_sim_uwb"), do_calib_imu_g_sensitivity=0, imu_model=imu_model,
                          max_msckf_in_update=60, max_slam_features=6, max_slam_in_update=3, dt_slam_delay=0.3,
                          min_dist_to_use_uwb=0.05)
    steps = _lockstep(opts, 10, anchors=True, spawn=40, frac_long=0.2)
    _check_lockstep(steps)
    kinds = steps[0][0]["meta"]
    assert int(kinds[0][2]) == 15 and int(kinds[:, 2].sum()) == steps[0][0]["P"].shape[0]
    N = max(a["timing"]["cov_dim"] for a, _ in steps)
    assert N >= 15 + 15 + 1 + 56 + 20 and N * 30 <= 8192
    assert _selector0(N, 30) == FUSED
    assert _selector0(N, 39) == SPLIT  # cfg5 itself (g-sensitivity on): always the three launches


# Both sides start from the same bits and evaluate the same formulas in float64; they differ in the order of the host's
# accumulation of Phi and Q over the ~11 IMU steps of a frame (15-term sums per step: ~2 * 11 * 15 u relative to the
# terms' magnitudes, on each side) and in the order of the covariance sums ((2 q + 4) u on each side, q = 15): about
# 730 u of the sums of magnitudes.  Those sums exceed the entries' own correlation scale sqrt(P_ii P_jj) where the
# position / velocity / orientation terms of mixed units cancel; 16 is allowed for that: 730 * 16 * 2^-53 = 1.3e-12,
# rounded up to 2^-38 = 3.6e-12.  (The max-norm bound of the lock-step runs, 1e-10 max |P|, is blind below the largest
# variance.)  Measured on MI355X: 2.7e-15 with and without the time offset; the marginalization after it: 0.
SCALED_BOUND = 2.0 ** -38


@pytest.mark.parametrize("calib_dt", [0, 1], ids=["nodt", "dt"])
def test_propagate_clone_marginalize_in_correlation_units(euroc_yaml, calib_dt):
    import uvio_amd as U
    from oracle import oracle as O
    from uvio_amd.sim import SimStream
    from test_gpu_updaters import _feed_imu_until, _sync
    opts = U.load_options(euroc_yaml, do_calib_camera_timeoffset=calib_dt, max_clone_size=5, max_msckf_in_update=40,
                          max_slam_features=0)
    n = 7
    sim = SimStream(opts, duration=(n + 4) / opts.track_frequency + 1.2, seed=13, spawn=30, frac_long=0.3)
    g, o = U.VioManager(opts), O.OracleManager(opts)
    try:
        sim.run([g, o], n_frames=n, before_frame=lambda nf, t: _sync(g, o))
        _sync(g, o)
        ct = g.get_clone_times()
        assert len(ct) == opts.max_clone_size
        meta = g.get_state_vector()[1]
        imu = int(meta[0][1])
        assert int(meta[0][2]) == 15
        i_next = int(np.argmin(np.abs(sim.cam_t - ct[-1]))) + 1
        t_next = float(sim.cam_t[i_next])
        _feed_imu_until(sim, [g, o], float(ct[-1]), t_next)
        N0 = g.cov_dim()
        P0 = g.get_cov()
        g.propagate_and_clone(t_next)
        o.propagate_and_clone(t_next)
        Pg, Po = g.get_cov(), o.get_cov()
        assert Pg.shape == Po.shape == (N0 + 6, N0 + 6)
        e1 = E.scaled_err(Pg, Po, Po)
        print("propagate_and_clone: scaled error %.3e (bound %.3e)" % (e1, SCALED_BOUND))
        assert e1 <= SCALED_BOUND, e1
        # The cross blocks against the new clone are bitwise symmetric on every row outside the IMU block: k_clone
        # writes column and row from P's column and row, which the propagation wrote from the same T.  (The
        # time-offset term adds P[i][dt] and P[dt][i], untouched by the propagation: equal when P was symmetric
        # before.)  The IMU block's own rows carry the block's asymmetry into the clone: only up to rounding there.
        out = np.r_[0:imu, imu + 15:N0]
        if not calib_dt or np.array_equal(P0, P0.T):
            assert R.same_bits(Pg[out, N0:], Pg[N0:, out].T)
        if not calib_dt:
            assert R.same_bits(Pg[N0:, N0:], Pg[imu:imu + 6, imu:imu + 6])
            assert R.same_bits(Pg[:N0, N0:], Pg[:N0, imu:imu + 6]) and R.same_bits(Pg[N0:, :N0], Pg[imu:imu + 6, :N0])
        else:
            assert not np.array_equal(Pg[N0:, N0:], Pg[imu:imu + 6, imu:imu + 6])
        _sync(g, o)
        g.marginalize_old_clone()
        o.marginalize_old_clone()
        Mg, Mo = g.get_cov(), o.get_cov()
        assert Mg.shape == Mo.shape == (N0, N0) and len(g.get_clone_times()) == opts.max_clone_size
        e2 = E.scaled_err(Mg, Mo, Mo)
        print("marginalize_old_clone: scaled error %.3e" % e2)
        assert e2 == 0.0  # a copy on both sides, from the same bits
    finally:
        g.close()
