"""The covariance bookkeeping kernels without a GPU: the float64 replay of tests/cov_ref.py against its longdouble
reference within a derived bound, the order-independence of a sequence of marginalizations on an asymmetric P, every
injected error caught by the comparison the GPU tests use (cov_ref.same_bits against the replay), and every refusal of
uvio_hp_debug_cov_propagate_p / uvio_hp_debug_cov_gather_p that needs no device.  The device's side is
tests/test_gpu_cov_ops.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cov_ref as R  # noqa: E402
import ekf_ref as E  # noqa: E402

needs_ld = pytest.mark.skipif(not E.HAVE_EXTENDED, reason=E.REASON)
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)

# (N, s0, p, q): the IMU block of cfg2-4, a p = 30 block, q != p on both sides, the largest block
SHAPES = [(40, 0, 15, 15), (64, 20, 30, 30), (64, 20, 9, 17), (64, 55, 9, 17), (64, 0, 17, 9), (33, 9, 6, 6),
          (300, 100, 64, 256), (5, 2, 1, 1)]


def _case(N, s0, p, q, seed=0):
    P = R.cov_case(N, 11 + N + seed)
    new = np.arange(s0, s0 + p)
    iold = R.iold_case(N, s0, p, q, 5 + seed)
    return P, new, iold, R.phi_case(new, iold, 17 + seed), R.q_case(p, 23 + seed)


def _rows_case(N, seed=0, zero_q=False):
    """variables of sizes 3, 1, 6 at non-adjacent positions, each row of Phi reading its own variable's columns and one
    shared column"""
    starts, sizes = (2, 11, N - 9), (3, 1, 6)
    rows = np.concatenate([np.arange(s, s + d) for s, d in zip(starts, sizes)]).astype(np.int32)
    shared = 7
    iold = np.concatenate([rows, [shared]]).astype(np.int32)
    Phi = R.phi_case(rows, iold, 31 + seed)
    at = 0
    for d in sizes:  # block rows: zero outside the variable's own columns and the shared one
        mask = np.ones(iold.size, dtype=bool)
        mask[at:at + d] = False
        mask[-1] = False
        Phi[at:at + d, mask] = 0.0
        at += d
    return R.cov_case(N, 41 + N + seed), rows, iold, Phi, R.q_case(rows.size, 43 + seed, zero=zero_q)


# ---- replay against the longdouble reference ----
@needs_ld
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-s%d-p%d-q%d" % s)
def test_propagate_replay_is_within_the_derived_bound(shape):
    P, new, iold, Phi, Q = _case(*shape)
    ref = R.propagate_ref(P, new, iold, Phi, Q)
    rep = R.propagate_replay64(P, new, iold, Phi, Q)
    bound = R.propagate_bound(P, new, iold, Phi, Q)
    err = np.abs(np.asarray(rep, dtype=E.LD) - ref)
    assert np.all(err <= bound), float(np.max(err / np.maximum(bound, E.LD(1e-300))))
    keep = np.setdiff1d(np.arange(P.shape[0]), new)
    assert R.same_bits(rep[np.ix_(keep, keep)], P[np.ix_(keep, keep)])  # untouched outside the block's rows / columns
    # the cross blocks are bitwise symmetric; the block itself only up to rounding
    assert R.same_bits(rep[np.ix_(keep, new)], rep[np.ix_(new, keep)].T)


def test_propagated_block_is_symmetric_only_up_to_rounding():
    """Phi P Phi^T is summed in two different orders for (x, a) and (a, x): the replay (and the reference's Eigen
    product) do not symmetrize it, so the triangle a later kernel reads is visible"""
    P, new, iold, Phi, Q = _case(40, 0, 15, 15)
    blk = R.propagate_replay64(P, new, iold, Phi, Q)[:15, :15]
    assert not np.array_equal(blk, blk.T) and np.allclose(blk, blk.T, rtol=1e-9, atol=0)


@needs_ld
@pytest.mark.parametrize("zero_q", [False, True], ids=["Q", "Q0"])
def test_rows_form_replay_is_within_the_derived_bound(zero_q):
    P, rows, iold, Phi, Q = _rows_case(40, zero_q=zero_q)
    ref = R.propagate_ref(P, rows, iold, Phi, Q)
    rep = R.propagate_replay64(P, rows, iold, Phi, Q)
    assert np.all(np.abs(np.asarray(rep, dtype=E.LD) - ref) <= R.propagate_bound(P, rows, iold, Phi, Q))
    # a block-row Phi: the contiguous propagation of one variable alone gives that variable's own block
    one = R.propagate_replay64(P, rows[:3], np.concatenate([rows[:3], iold[-1:]]), Phi[:3, [0, 1, 2, -1]],
                               R.sym_upper(Q)[:3, :3])
    assert np.array_equal(one[np.ix_(rows[:3], rows[:3])], rep[np.ix_(rows[:3], rows[:3])])


@needs_ld
@pytest.mark.parametrize("dt_id", [-1, 3, 30], ids=["nodt", "dt-before", "dt-after"])
def test_clone_replay_is_within_the_derived_bound(dt_id):
    P, new, iold, Phi, Q = _case(40, 9, 15, 15)
    Pp = R.propagate_replay64(P, new, iold, Phi, Q)
    dnc = np.array([0.3, -0.02, 1e-3, -1.5, 0.25, 4.0])
    ref = R.clone_ref(Pp, 9, dt_id, dnc)
    rep = R.clone_replay64(Pp, 9, dt_id, dnc)
    assert np.all(np.abs(np.asarray(rep, dtype=E.LD) - ref) <= R.clone_bound(Pp, 9, dt_id, dnc))
    assert R.same_bits(rep[:40, :40], Pp)
    if dt_id < 0:  # a copy: the clone block equals the pose block entry for entry
        assert R.same_bits(rep[40:, 40:], Pp[9:15, 9:15]) and R.same_bits(rep, np.asarray(ref, dtype=np.float64))
    else:
        assert not np.array_equal(rep[40:, 40:], Pp[9:15, 9:15])


# ---- marginalization ----
VARS = [(0, 6), (6, 3), (14, 1), (20, 6), (27, 3)]  # the first variable, an adjacent pair, the last variable of N = 30


@pytest.mark.parametrize("pick", [(0, 1), (2, 4), (0, 1, 2), (1, 3, 4), (0, 1, 3, 4), (0, 2, 3, 4)],
                         ids=lambda v: "v" + "".join(map(str, v)))
def test_every_order_of_the_sequence_gives_the_same_matrix(pick):
    P = R.coded(30)
    variables = [VARS[k] for k in pick]
    src = R.kept_indices(30, variables)
    first = R.marginalize_seq(P, variables)
    for order in R.all_orders(len(variables)):
        assert np.array_equal(R.marginalize_seq(P, variables, order), first), order
    # ... and it is the kernel's flip rule, which on this P differs from the plain gather exactly where it flips
    assert np.array_equal(R.marginalize_multi_model(P, src), first)
    plain = P[np.ix_(src, src)]
    assert np.array_equal(plain != first, R.flip_mask(src))
    assert R.flip_mask(src).any() == (pick != (0, 1))  # (nothing kept lies before the two leading variables)
    assert np.array_equal(R.marginalize_multi_model(R.coded(30, True), src), R.coded(30, True)[np.ix_(src, src)])


def test_marginalize_one_reads_the_upper_right_block():
    P = R.coded(12)
    out = R.marginalize_one(P, 4, 3)
    keep = np.r_[0:4, 7:12]
    want = P[np.ix_(keep, keep)]
    want[4:, :4] = P[np.ix_(np.arange(4), np.arange(7, 12))].T
    assert np.array_equal(out, want) and not np.array_equal(out, P[np.ix_(keep, keep)])
    assert np.array_equal(R.marginalize_one(P, 0, 12).shape, (0, 0))
    assert np.array_equal(R.marginalize_one(P, 9, 3), P[:9, :9]) and np.array_equal(R.marginalize_one(P, 0, 2), P[2:, 2:])


# ---- every injected error fails the GPU tests' comparison ----
def test_injected_propagation_errors_are_caught():
    P, new, iold, Phi, Q = _case(64, 20, 9, 9)
    want = R.expected_buffer(P, new, iold, Phi, Q, ld=70)

    def buf(out):
        b = np.full((64, 70), R.NAN_FILL)
        b[:, :64] = out
        return b

    assert R.same_bits(buf(R.propagate_replay64(P, new, iold, Phi, Q)), want)
    assert not R.same_bits(buf(R.propagate_replay64(P, new, iold, Phi.T, Q)), want)            # Phi transposed
    assert not R.same_bits(buf(R.propagate_replay64(P, new, np.roll(iold, 1), Phi, Q)), want)  # iold permuted
    assert not R.same_bits(buf(R.propagate_replay64(P, new, iold, Phi, Q.T)), want)            # Q's lower triangle read
    # a different summation order (descending b) is seen too: the comparison is to the last bit
    rev = R.propagate_replay64(P, new, iold[::-1], Phi[:, ::-1], Q)
    assert not R.same_bits(buf(rev), want) and np.allclose(rev, want[:, :64], rtol=1e-9, atol=0)
    # the padding: one payload bit of one padding entry
    b = want.copy()
    b.view(np.uint64)[3, 66] ^= np.uint64(2)
    assert not R.same_bits(b, want) and np.array_equal(b, want, equal_nan=True)


def _clone_mutants(Pp, src0, dt_id, d):
    N = Pp.shape[0]
    S = slice(src0, src0 + 6)
    good = R.clone_replay64(Pp, src0, dt_id, d)
    col, row, b1, b2, swap = (good.copy() for _ in range(5))
    col[:N, N:] = Pp[:, S]                                                            # term dropped from the columns
    row[N:, :N] = Pp[S, :]                                                            # ... from the rows
    b1[N:, N:] = Pp[S, S] + d[:, None] * (Pp[dt_id, S][None, :] + Pp[dt_id, dt_id] * d[None, :])  # ... P[S a][dt] d[b]
    b2[N:, N:] = Pp[S, S] + Pp[S, dt_id][:, None] * d[None, :]                         # ... d[a] (..)
    swap[:N, N:], swap[N:, :N] = good[N:, :N].T, good[:N, N:].T                        # row and column swapped
    return good, {"col": col, "row": row, "block-1": b1, "block-2": b2, "swapped": swap}


@pytest.mark.parametrize("dt_id", [3, 30])
def test_injected_clone_errors_are_caught(dt_id):
    P, new, iold, Phi, Q = _case(40, 9, 15, 15)
    Pp = R.propagate_replay64(P, new, iold, Phi, Q)
    good, mutants = _clone_mutants(Pp, 9, dt_id, np.array([0.3, -0.02, 1e-3, -1.5, 0.25, 4.0]))
    for name, bad in mutants.items():
        assert not R.same_bits(bad, good), name
    # without the term the swap is still seen, through the asymmetry of the propagated block alone
    plain = R.clone_replay64(Pp, 9)
    swapped = plain.copy()
    swapped[:40, 40:], swapped[40:, :40] = plain[40:, :40].T, plain[:40, 40:].T
    assert not R.same_bits(swapped, plain)


def test_injected_marginalization_errors_are_caught():
    P = R.coded(30)
    variables = [VARS[0], VARS[2], VARS[4]]
    src = R.kept_indices(30, variables)
    want = R.marginalize_seq(P, variables)
    assert np.array_equal(R.marginalize_multi_model(P, src, "rule"), want)
    assert not np.array_equal(R.marginalize_multi_model(P, src, "inverted"), want)
    assert not np.array_equal(R.marginalize_multi_model(P, src, "dropped"), want)
    # the single kernel's cross block taken from P's own lower-left
    keep = np.r_[0:14, 15:30]
    assert not np.array_equal(P[np.ix_(keep, keep)], R.marginalize_one(P, 14, 1))
    # on a symmetric P none of these shows: the reason the asymmetric one is used
    Ps = R.coded(30, True)
    assert np.array_equal(R.marginalize_multi_model(Ps, src, "dropped"), R.marginalize_seq(Ps, variables))


# ---- exports and refusals ----
def test_library_exports_the_two_entries():
    from uvio_amd import _native as N
    lib = N.load()
    for name in ("debug_cov_propagate_p", "debug_cov_gather_p"):
        assert hasattr(lib, "uvio_hp_" + name) and "uvio_hp_" + name in N.EXPORTED, name
    assert (N.COV_PATH_AUTO, N.COV_PATH_SPLIT, N.COV_PATH_FUSED) == (0, 1, 2)


def _ptr(a, t=dp):
    return None if a is None else a.ctypes.data_as(t)


def test_propagate_refusals_need_no_device():
    """every argument check of uvio_hp_debug_cov_propagate_p comes before the device is touched and leaves P alone"""
    from uvio_amd import _native as N
    f = N.load().uvio_hp_debug_cov_propagate_p
    P0 = np.full((26, 30), 3.5)
    base = dict(P=P0, N=20, ld=30, s0=4, p=3, rows=None, iold=np.array([4, 5, 6, 9], dtype=np.int32), q=4,
                Phi=np.ones((3, 4)), Q=np.eye(3), clone=1, src0=2, dt_id=10, dnc=np.ones(6), path=0)

    def call(**kw):
        a = dict(base, **kw)
        Pc = None if a["P"] is None else np.array(a["P"])
        ran = C.c_int(-9)
        rc = f(_ptr(Pc), a["N"], a["ld"], a["s0"], a["p"], _ptr(a["rows"], ip), _ptr(a["iold"], ip), a["q"],
               _ptr(a["Phi"]), _ptr(a["Q"]), a["clone"], a["src0"], a["dt_id"], _ptr(a["dnc"]), a["path"],
               None if kw.get("no_ran") else C.byref(ran))
        assert ran.value == -9 and (Pc is None or np.array_equal(Pc, P0))
        return rc

    for null in ("P", "iold", "Phi", "Q", "dnc"):
        assert call(**{null: None}) == N.E_ARG, null
    assert call(no_ran=True) == N.E_ARG
    assert call(dnc=None, dt_id=-1, ld=25) == N.E_ARG                      # ld < N + 6 with a clone
    assert call(clone=0, ld=19) == N.E_ARG                                 # ld < N without one
    assert call(N=0) == N.E_ARG and call(p=0) == N.E_ARG and call(q=0) == N.E_ARG
    assert call(s0=-1) == N.E_ARG and call(s0=18) == N.E_ARG               # the block outside [0, N)
    assert call(iold=np.array([4, 5, 6, 20], dtype=np.int32)) == N.E_ARG   # a column outside [0, N)
    assert call(iold=np.array([4, -1, 6, 9], dtype=np.int32)) == N.E_ARG
    assert call(iold=np.array([4, 5, 4, 9], dtype=np.int32)) == N.E_ARG    # a repeated column
    assert call(src0=-1) == N.E_ARG and call(src0=15) == N.E_ARG           # the pose outside [0, N)
    assert call(dt_id=20) == N.E_ARG
    rows = np.array([1, 7, 12], dtype=np.int32)
    assert call(rows=rows) == N.E_ARG                                      # rows together with a clone
    assert call(rows=np.array([1, 7, 20], dtype=np.int32), clone=0) == N.E_ARG
    assert call(rows=np.array([1, 7, 7], dtype=np.int32), clone=0) == N.E_ARG
    assert call(path=3) == N.E_ARG and call(path=-1) == N.E_ARG
    assert call(path=2, clone=0) == N.E_ARG                                # the fused kernel is propagation + clone
    # capacity: Engine::cov_propagate's limits, and the fused kernel's
    big = np.full((306, 306), 3.5)

    def cap(p, q, n=300, path=0):
        Pc = big.copy()
        ran = C.c_int(-9)
        rc = f(_ptr(Pc), n, 306, 0, p, None, _ptr(np.arange(q, dtype=np.int32), ip), q, _ptr(np.zeros((p, q))),
               _ptr(np.zeros((p, p))), 1, 0, -1, None, path, C.byref(ran))
        assert ran.value == -9 and np.array_equal(Pc, big)
        return rc

    assert cap(65, 8) == N.E_CAPACITY and cap(8, 257) == N.E_CAPACITY
    assert cap(33, 33, n=100, path=2) == N.E_CAPACITY and cap(15, 33, n=100, path=2) == N.E_CAPACITY
    assert cap(15, 15, n=547, path=2) == N.E_ARG                           # (N + 6 > ld comes first)
    wide = np.full((553, 553), 3.5)
    ran = C.c_int(-9)
    args = (547, 553, 0, 15, None, _ptr(np.arange(15, dtype=np.int32), ip), 15, _ptr(np.zeros((15, 15))),
            _ptr(np.zeros((15, 15))), 1, 0, -1, None, 2, C.byref(ran))
    assert f(_ptr(wide), *args) == N.E_CAPACITY and ran.value == -9        # N p = 8205 > 8192
    assert f(_ptr(np.full((306, 306), 3.5)), 274, 306, 0, 30, None, _ptr(np.arange(30, dtype=np.int32), ip), 30,
             _ptr(np.zeros((30, 30))), _ptr(np.zeros((30, 30))), 1, 0, -1, None, 2, C.byref(ran)) == N.E_CAPACITY


def test_gather_refusals_need_no_device_and_an_empty_result_succeeds():
    from uvio_amd import _native as N
    f = N.load().uvio_hp_debug_cov_gather_p
    P = R.coded(12)
    out0 = np.full((12, 12), -1.0)
    idx = np.array([0, 3, 4, 9], dtype=np.int32)

    def call(P_=P, N_=12, ld=12, op=N.COV_MARGINALIZE, m0=2, ms=3, idx_=idx, n=4, out_=out0):
        o = None if out_ is None else out_.copy()
        rc = f(_ptr(P_), N_, ld, op, m0, ms, _ptr(idx_, ip), n, _ptr(o))
        assert o is None or np.array_equal(o, out0)
        return rc

    assert call(P_=None) == N.E_ARG and call(out_=None) == N.E_ARG
    assert call(ld=11) == N.E_ARG and call(N_=0) == N.E_ARG
    assert call(op=4) == N.E_ARG and call(op=-1) == N.E_ARG
    assert call(m0=-1) == N.E_ARG and call(ms=0) == N.E_ARG and call(m0=10) == N.E_ARG
    for op in (N.COV_MARGINALIZE_MULTI, N.COV_COMPACT, N.COV_MARGINAL_GATHER):
        assert call(op=op, idx_=None) == N.E_ARG and call(op=op, n=-1) == N.E_ARG
        assert call(op=op, idx_=np.array([0, 3, 12, 9], dtype=np.int32)) == N.E_ARG
        assert call(op=op, idx_=np.array([0, -1, 4, 9], dtype=np.int32)) == N.E_ARG
        assert call(op=op, n=0) == 0 and call(op=op, n=0, idx_=None) == 0        # nothing to launch
    assert call(op=N.COV_MARGINALIZE_MULTI, idx_=np.array([0, 4, 3, 9], dtype=np.int32)) == N.E_ARG  # not ascending
    assert call(op=N.COV_MARGINALIZE_MULTI, idx_=np.array([0, 3, 3, 9], dtype=np.int32)) == N.E_ARG
    many = np.zeros(4097, dtype=np.int32)
    assert call(op=N.COV_COMPACT, idx_=many, n=13) == N.E_ARG
    assert call(op=N.COV_MARGINAL_GATHER, idx_=many, n=4097) == N.E_CAPACITY
    assert call(m0=0, ms=12) == 0                                                 # everything removed: Nn = 0


def test_valid_calls_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import uvio_amd as U
    from uvio_amd import _native as N
    P, new, iold, Phi, Q = _case(40, 0, 15, 15)
    with pytest.raises(RuntimeError, match="E_DEVICE"):
        U.cov_propagate_p(P, 0, iold, Phi, Q, clone_src=0)
    with pytest.raises(RuntimeError, match="E_DEVICE"):
        U.cov_gather_p(R.coded(12), N.COV_MARGINALIZE, m0=2, ms=3)
    assert U.cov_gather_p(R.coded(12), N.COV_MARGINALIZE, m0=0, ms=12).shape == (0, 12)
