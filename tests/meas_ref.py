"""StateHelper::EKFUpdate with a dense noise matrix, restated in NumPy for the measurement-update tests
(tests/test_meas_ref.py, tests/test_gpu_meas_update.py).  NumPy only: nothing from oracle/ or uvio_amd/.

    S = H P_II H^T + R = L L^T,  W = P[:, I] H^T L^-T,  P+ = P - W W^T,  dx = W L^-1 res,  chi2 = |L^-1 res|^2

Only R's upper triangle is read (the reference: S.triangularView<Upper>() += R, then S.selfadjointView<Upper>()).
In numpy.longdouble this is the reference (ekf_ref.HAVE_EXTENDED says whether longdouble is good for that here);
in float64 it is the comparator whose own error against the reference scales the device's bound.
"""
from collections import namedtuple

import numpy as np

import ekf_ref as E

LD = E.LD


def _chol(A):
    n = A.shape[0]
    L = np.zeros((n, n), dtype=A.dtype)
    for j in range(n):
        c = A[j:, j] - L[j:, :j] @ L[j, :j]
        assert c[0] > 0, ("not positive definite at column", j, float(c[0]))
        L[j, j] = np.sqrt(c[0])
        L[j + 1:, j] = c[1:] / L[j, j]
    return L


def _fwd(L, B):
    X = np.array(B, dtype=L.dtype)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def ekf_update_R_ref(P, idx, H, res, R, dtype=LD):
    """(P_plus, dx, chi2) in `dtype` arithmetic; R's strictly lower triangle is never read."""
    P = np.asarray(P, dtype=dtype)
    H = np.asarray(H, dtype=dtype)
    res = np.asarray(res, dtype=dtype)
    idx = np.asarray(idx, dtype=np.intp)
    m, n = H.shape
    assert idx.shape == (n,) and res.shape == (m,) and np.shape(R) == (m, m)
    Ru = np.triu(np.asarray(R, dtype=dtype))
    Rs = Ru + np.triu(Ru, 1).T
    T = H @ P[idx, :]  # m x N
    S = T[:, idx] @ H.T
    S = (S + S.T) / 2 + Rs
    L = _chol(S)
    Wt = _fwd(L, T)
    y = _fwd(L, res)
    return P - Wt.T @ Wt, Wt.T @ y, y @ y


MCase = namedtuple("MCase", "P idx H res R")


def dense_R(r, rng, lo=-1.5, hi=0.5):
    """SPD and dense: D (A A^T / r + 1e-3 I) D with D a random permutation of logspace(lo, hi, r), so the variances
    span 2 (hi - lo) orders of magnitude around the order-one H P_II H^T of ekf_ref.graded_case; exactly symmetric."""
    D = np.logspace(lo, hi, r)[rng.permutation(r)]
    A = rng.standard_normal((r, r))
    R = (A @ A.T / r + 1e-3 * np.eye(r)) * np.outer(D, D)
    return np.triu(R) + np.triu(R, 1).T


def graded_R_case(N, n, r, seed):
    """ekf_ref.graded_case's P, idx, H, res with a dense graded R in place of sigma2 I"""
    k = E.graded_case(N, n, r, seed, 1.0, full=(n == N))
    return MCase(k.P, k.idx, k.H, k.res, dense_R(r, np.random.default_rng(seed + 7919)))


# (N, n, r) at the factor kernel's dispatch edges: one panel wave up to r = 63, LDS up to 137, global from 138, the
# largest panel; N = 15 / 16 / 17 / 41 around the 16-row tiles of P
SHAPES = [(15, 1, 1), (16, 6, 3), (17, 6, 6), (41, 24, 16), (41, 24, 17), (80, 70, 63), (80, 70, 64), (150, 140, 137),
          (150, 140, 138), (272, 255, 255)]


def shape_id(s):
    return "N%d-n%d-r%d" % tuple(s)


def shape_seed(s):
    return 4000 + 7 * s[0] + 3 * s[1] + s[2]


# ---- the worked measurement: a position sensor on a lever arm ----
def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]], dtype=np.asarray(v).dtype)


def quat_2_Rot(q):
    """JPL (x, y, z, w): R = (2 w^2 - 1) I - 2 w [q_v]x + 2 q_v q_v^T"""
    q = np.asarray(q)
    return (2 * q[3] * q[3] - 1) * np.eye(3, dtype=q.dtype) - 2 * q[3] * skew(q[:3]) + 2 * np.outer(q[:3], q[:3])


def quat_multiply(q, p):
    """JPL q (x) p (ov_core quat_ops.h quat_multiply)"""
    Qm = np.zeros((4, 4), dtype=np.asarray(q).dtype)
    Qm[:3, :3] = q[3] * np.eye(3) - skew(q[:3])
    Qm[:3, 3] = q[:3]
    Qm[3, :3] = -q[:3]
    Qm[3, 3] = q[3]
    out = Qm @ p
    if out[3] < 0:
        out = -out
    return out / np.linalg.norm(out)


def quat_boxplus(q, dth):
    """JPLQuat::update: [dth / 2, 1] normalized, times q"""
    dq = np.concatenate([0.5 * np.asarray(dth), [1.0]]).astype(np.asarray(q).dtype)
    dq = dq / np.linalg.norm(dq)
    return quat_multiply(dq, q)


def position_h(q, p, p_SinI):
    return np.asarray(p) + quat_2_Rot(q).T @ np.asarray(p_SinI)
