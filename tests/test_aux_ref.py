"""Caller-defined state variables without a GPU: the library exports the uvio_hp_aux_* entries and every refusal that
needs no device answers on a host without one; the NumPy reference (tests/aux_ref.py) is held against itself; the
lever-arm Jacobian of the Python mirror is compared with finite differences.  The device's side is
tests/test_gpu_aux_state.py, the C++ facade's tests/test_facade_aux.py."""
import ctypes as C
import os
import shutil
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import aux_ref as A  # noqa: E402
import ekf_ref as E  # noqa: E402
import meas_ref as M  # noqa: E402

needs_ld = pytest.mark.skipif(not E.HAVE_EXTENDED, reason=E.REASON)
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


# ---- exports, the option, refusals ----
def test_library_exports_the_aux_entries_and_the_option(euroc_yaml, tmp_path):
    from uvio_amd import _native as N
    import uvio_amd as U
    lib = N.load()
    for name in ("aux_add", "aux_add_from_measurement", "aux_get", "aux_remove", "aux_count", "aux_append_p",
                 "aux_init_p", "aux_walk_p"):
        assert hasattr(lib, "uvio_hp_" + name) and "uvio_hp_" + name in N.EXPORTED, name
    assert N.Options._fields_[-1][0] == "max_aux_dim" and N.AUX_MAX_DIM == 8
    assert U.load_options().max_aux_dim == 0 and U.load_options(euroc_yaml).max_aux_dim == 0
    # the loader reads a key of the same name: a copy of the configuration with it appended
    d = tmp_path / "cfg"
    shutil.copytree(os.path.dirname(euroc_yaml), d)
    with open(d / os.path.basename(euroc_yaml), "a") as f:
        f.write("\nmax_aux_dim: 5\n")
    assert U.load_options(str(d / os.path.basename(euroc_yaml))).max_aux_dim == 5


def test_handle_entries_refuse_a_null_handle():
    from uvio_amd import _native as N
    lib = N.load()
    one, h = np.ones(1), C.c_int(-3)
    assert lib.uvio_hp_aux_add(None, 1, one.ctypes.data_as(dp), one.ctypes.data_as(dp), 1, None, C.byref(h)) == N.E_ARG
    assert lib.uvio_hp_aux_add_from_measurement(None, 1, one.ctypes.data_as(dp), 0, None, None, None, 1,
                                                one.ctypes.data_as(dp), 1, one.ctypes.data_as(dp),
                                                one.ctypes.data_as(dp), 1, None, C.byref(h)) == N.E_ARG
    assert lib.uvio_hp_aux_get(None, 1, C.byref(h), C.byref(h), None) == N.E_ARG
    assert lib.uvio_hp_aux_remove(None, 1) == N.E_ARG
    assert lib.uvio_hp_aux_count(None, C.byref(h), C.byref(h)) == N.E_ARG
    assert h.value == -3


def _raw(fn, P, *args):
    """a twin on a copy of P: (status, P unchanged?)"""
    Pc = np.array(P, dtype=np.float64)
    rc = fn(Pc.ctypes.data_as(dp), *args)
    return rc, np.array_equal(Pc, P, equal_nan=True)


def test_standalone_refusals_need_no_device():
    """every argument check of the three twins comes before the device is touched and leaves P alone"""
    from uvio_amd import _native as N
    lib = N.load()
    P = np.full((8, 8), 3.5)
    pr = np.eye(3)
    f = lib.uvio_hp_aux_append_p
    prp = pr.ctypes.data_as(dp)
    assert _raw(f, P, 5, 8, 0, prp, 3) == (N.E_ARG, True)      # dim outside 1 .. 8
    assert _raw(f, P, 5, 8, 9, prp, 9) == (N.E_ARG, True)
    assert _raw(f, P, 6, 8, 3, prp, 3) == (N.E_ARG, True)      # N + dim > ld
    assert _raw(f, P, 5, 8, 3, prp, 2) == (N.E_ARG, True)      # leading dimension below the row length
    assert _raw(f, P, -1, 8, 3, prp, 3) == (N.E_ARG, True)
    assert _raw(f, P, 5, 8, 3, None, 3) == (N.E_ARG, True)
    assert f(None, 5, 8, 3, prp, 3) == N.E_ARG
    for bad in (np.diag([1.0, 0.0, 1.0]), np.diag([1.0, -2.0, 1.0]), np.triu(np.full((3, 3), np.nan)),
                np.eye(3) + np.triu(np.full((3, 3), np.inf), 1)):
        assert _raw(f, P, 5, 8, 3, bad.ctypes.data_as(dp), 3) == (N.E_ARG, True)
    g = lib.uvio_hp_aux_init_p
    idx = np.array([4, 0, 2], dtype=np.int32)
    Hx, Hi, R = np.ones((3, 3)), np.eye(3), np.eye(3)

    def init(N_=5, ld=8, dim=3, idx_=idx, n=3, Hx_=Hx, ldhx=3, Hi_=Hi, R_=R, ldr=3):
        return _raw(g, P, N_, ld, dim, None if idx_ is None else idx_.ctypes.data_as(ip), n,
                    None if Hx_ is None else Hx_.ctypes.data_as(dp), ldhx, None if Hi_ is None else Hi_.ctypes.data_as(dp),
                    None, None if R_ is None else R_.ctypes.data_as(dp), ldr)

    assert init(dim=0) == (N.E_ARG, True) and init(dim=9) == (N.E_ARG, True)
    assert init(N_=6) == (N.E_ARG, True)
    assert init(ldhx=2) == (N.E_ARG, True) and init(ldr=2) == (N.E_ARG, True)
    assert init(idx_=np.array([4, 5, 2], dtype=np.int32)) == (N.E_ARG, True)   # a column outside [0, N)
    assert init(idx_=np.array([4, -1, 2], dtype=np.int32)) == (N.E_ARG, True)
    assert init(idx_=None) == (N.E_ARG, True) and init(Hi_=None) == (N.E_ARG, True) and init(R_=None) == (N.E_ARG, True)
    assert init(Hx_=np.array([[1.0, np.nan, 1.0]] * 3)) == (N.E_ARG, True)
    assert init(Hi_=np.diag([1.0, np.inf, 1.0])) == (N.E_ARG, True)
    assert init(R_=np.triu(np.full((3, 3), np.nan))) == (N.E_ARG, True)
    big = np.zeros(1216, dtype=np.int32)
    Pb = np.zeros((4, 4))
    Hb = np.zeros((1, 1216))
    one = np.ones((1, 1))
    assert _raw(g, Pb, 3, 4, 1, big.ctypes.data_as(ip), 1216, Hb.ctypes.data_as(dp), 1216, one.ctypes.data_as(dp), None,
                one.ctypes.data_as(dp), 1) == (N.E_CAPACITY, True)
    w = lib.uvio_hp_aux_walk_p
    ids, dims, s2 = np.array([1, 5], dtype=np.int32), np.array([2, 3], dtype=np.int32), np.ones(5)

    def walk(N_=8, ld=8, ids_=ids, dims_=dims, s2_=s2, dt=0.1):
        return _raw(w, P, N_, ld, len(ids_), ids_.ctypes.data_as(ip), dims_.ctypes.data_as(ip), s2_.ctypes.data_as(dp), dt)

    assert walk(ld=7) == (N.E_ARG, True)
    assert walk(dt=-0.1) == (N.E_ARG, True) and walk(dt=float("nan")) == (N.E_ARG, True)
    assert walk(ids_=np.array([1, 6], dtype=np.int32)) == (N.E_ARG, True)       # a block outside [0, N)
    assert walk(ids_=np.array([1, 2], dtype=np.int32)) == (N.E_ARG, True)       # overlapping blocks
    assert walk(dims_=np.array([2, 9], dtype=np.int32)) == (N.E_ARG, True)
    assert walk(s2_=np.array([1.0, -1.0, 1.0, 1.0, 1.0])) == (N.E_ARG, True)
    assert walk(s2_=np.array([1.0, np.nan, 1.0, 1.0, 1.0])) == (N.E_ARG, True)


def test_valid_standalone_calls_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import uvio_amd as U
    # a NaN below the diagonals is not an argument error: those triangles are never read
    low = np.tril(np.full((2, 2), np.nan), -1)
    with pytest.raises(RuntimeError, match="E_DEVICE"):
        U.aux_append_p(np.eye(3), np.eye(2) + low)
    with pytest.raises(RuntimeError, match="E_DEVICE"):
        U.aux_init_p(np.eye(3), [2, 0], np.ones((2, 2)), np.eye(2), np.eye(2) + low)
    with pytest.raises(RuntimeError, match="E_DEVICE"):
        U.aux_walk_p(np.eye(3), [1], [2], [1.0, 2.0], 0.5)


# ---- the NumPy reference held against itself ----
SMALL = [(5, 1, 1), (17, 3, 6), (70, 8, 65), (40, 3, 130)]


@pytest.mark.parametrize("dtype", [np.float64, E.LD], ids=["f64", "ld"])
def test_prior_only_append_is_the_zero_Hx_case(dtype):
    """initialize_invertible with H_x = 0 and H_aux = I leaves no correlation and the block R: that is the append"""
    P, _ = A.spd_case(17, 5)
    prior = A.init_case(17, 3, 6, 6)[5]
    idx = np.array([3, 11, 0, 9], dtype=np.int32)
    got = A.init_ref(P, idx, np.zeros((3, 4)), np.eye(3), prior, dtype)
    assert np.array_equal(got, A.append_ref(P, prior, dtype))
    assert np.array_equal(A.init_ref(P, idx[:0], np.zeros((3, 0)), np.eye(3), prior, dtype), A.append_ref(P, prior, dtype))
    if dtype is np.float64:
        rep = A.init_replay64(P, idx, np.zeros((3, 4)), np.eye(3), prior)
        assert np.array_equal(rep, got) and not np.any(np.signbit(rep[:17, 17:]))


@needs_ld
@pytest.mark.parametrize("s", SMALL, ids=lambda s: "N%d-d%d-n%d" % s)
def test_initialized_block_is_symmetric_and_positive_definite(s):
    N, d, n = s
    P, idx, Hx, Haux, Hinv, R = A.init_case(N, d, n, 100 + N)
    ref = A.init_ref(P, idx, Hx, Hinv, R)
    rep = A.init_replay64(P, idx, Hx, Hinv, R)
    for X in (ref, rep):
        assert np.array_equal(X, X.T)
        assert np.array_equal(np.asarray(X[:N, :N], dtype=np.float64), P)
    # positive definite for a positive definite P and R: the Schur complement of P in the augmented matrix is
    # H_aux^-1 R H_aux^-T; the Cholesky factor in longdouble exists
    E.chol_ld(ref)
    # the float64 comparator is the reference up to float64 rounding of sums of n order-one terms: n * 2^-52 in
    # correlation units, times the growth through H_aux^-1 (cond <= 8 here): 1e-12 is two orders above that
    e = A.scaled_err_new(rep, ref)
    assert e < 1e-12, e


@pytest.mark.parametrize("dtype", [np.float64, E.LD], ids=["f64", "ld"])
def test_lower_triangles_of_prior_and_R_are_never_read(dtype):
    P, idx, Hx, Haux, Hinv, R = A.init_case(17, 3, 6, 9)
    low = np.tril(np.full((3, 3), np.nan), -1)
    assert np.array_equal(A.append_ref(P, R + low, dtype), A.append_ref(P, R, dtype))
    assert np.array_equal(A.init_ref(P, idx, Hx, Hinv, R + low, dtype), A.init_ref(P, idx, Hx, Hinv, R, dtype))
    assert np.array_equal(A.init_replay64(P, idx, Hx, Hinv, R + low), A.init_replay64(P, idx, Hx, Hinv, R))
    # a leading dimension wider than d
    Rw = np.full((3, 5), np.nan)
    Rw[:, :3] = np.triu(R) + low
    assert np.array_equal(A.init_ref(P, idx, Hx, Hinv, Rw, dtype), A.init_ref(P, idx, Hx, Hinv, R, dtype))


def test_lane_sum_is_a_sum_and_the_walk_replay_rounds_twice():
    rng = np.random.default_rng(3)
    for n in (0, 1, 63, 64, 65, 200):
        x = rng.standard_normal((4, n))
        assert np.max(np.abs(A.lane_sum(x) - x.sum(axis=1))) <= 1e-13
    # one term per lane and nothing else: the sum of a single term is the term
    assert A.lane_sum(np.array([0.1]))[()] == 0.1
    P = np.diag([1.0, 1e-8, 3.0])
    s2, dt = np.array([0.1 * 0.1, 1e-3 * 1e-3]), 0.05000000000000071
    out = A.walk_replay64(P, [0, 1], s2, dt)
    for j in range(2):
        assert out[j, j] == P[j, j] + np.float64(s2[j] * dt)
    assert out[2, 2] == 3.0 and np.count_nonzero(out - np.diag(np.diag(out))) == 0
    if E.HAVE_EXTENDED:
        assert np.max(np.abs(A.walk_ref(P, [0, 1], s2, dt) - out)) <= 2.0 ** -52  # one rounding of a sum in [1, 2)


# ---- the lever-arm Jacobian ----
def lever_arm_h(q, p, arm):
    """z = p_IinG + R_ItoG p_AinI"""
    return M.position_h(q, p, arm)


def fd_lever_arm_jacobian(q, p, arm):
    """central differences of z over [dtheta (JPL left), dp, dp_AinI] in longdouble: step 1e-6, truncation
    O(step^2) = 1e-12, rounding eps_ld / step = 1e-13 (tests/test_meas_ref.py's procedure)"""
    LD = E.LD
    q, p, arm = np.asarray(q, dtype=LD), np.asarray(p, dtype=LD), np.asarray(arm, dtype=LD)
    step = LD(1e-6)
    J = np.zeros((3, 9), dtype=LD)
    for j in range(9):
        d = np.zeros(9, dtype=LD)
        d[j] = step
        hp = lever_arm_h(M.quat_boxplus(q, d[:3]), p + d[3:6], arm + d[6:])
        hm = lever_arm_h(M.quat_boxplus(q, -d[:3]), p - d[3:6], arm - d[6:])
        J[:, j] = (hp - hm) / (2 * step)
    return J


def random_poses(k=4, seed=21):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        q = rng.standard_normal(4)
        out.append((q / np.linalg.norm(q), 5.0 * rng.standard_normal(3), rng.uniform(-1.0, 1.0, 3)))
    return out


@needs_ld
def test_lever_arm_jacobian_python_mirror_matches_finite_differences():
    from uvio_amd.manager import position_fix_lever_arm_jacobian
    for q, p, arm in random_poses():
        h, H = position_fix_lever_arm_jacobian(q, p, arm)
        assert H.shape == (3, 9)
        assert np.max(np.abs(h - lever_arm_h(q, p, arm))) < 1e-14
        assert np.max(np.abs(H - fd_lever_arm_jacobian(q, p, arm))) < 1e-10
        # the aux block is R_ItoG
        assert np.max(np.abs(H[:, 6:] - M.quat_2_Rot(q).T)) < 1e-15
