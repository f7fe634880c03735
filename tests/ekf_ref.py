"""Extended-precision (numpy.longdouble, 64-bit mantissa) restatement of StateHelper::EKFUpdate and of the
measurement-compression Gram, the reference of tests/test_ekf_ref.py and tests/test_gpu_ekf_paths.py.  NumPy
only: nothing from oracle/ or uvio_amd/.

  * m <= n (direct form):   S = H P_II H^T + sigma2 I = L L^T,  W = P[:, I] H^T L^-T,
                            P+ = P - W W^T,  dx = W L^-1 res
  * m >  n (Gram form):     P_II = L L^T,  Z = L^T (H^T H) L + sigma2 I = U U^T,  V = P[:, I] L^-T,  X = V U^-T,
                            P+ = P - V V^T + sigma2 X X^T,  dx = X U^-1 L^T H^T res
    (with A = H L: H^T S^-1 H = L^-T A^T (A A^T + sigma2 I)^-1 A L^-1 = L^-T (I - sigma2 Z^-1) L^-1)

Both are the same map P, H, res -> P+, dx; tests/test_ekf_ref.py holds them against each other.

The error metrics divide by the prior standard deviations: |dP_ij| / sqrt(P_ii P_jj) is an error in correlation
units, in which a wrong digit in a block of small variances (biases, time offset: 1e-8 .. 1e-6 next to landmarks
at 1e-2 .. 1) is as visible as one in the largest block; max|dP| / max|P| does not see such a block at all.

graded_case is the one input generator of the CPU and the GPU tests, and DIRECT_CASES / INFO_CASES / GRAM_CASES
the one case list: the sizes are the dispatch boundaries of the device's factor kernels (panel waves, LDS /
packed / split storage, Gram chunking), see tests/test_gpu_ekf_paths.py.
"""
from collections import namedtuple

import numpy as np

LD = np.longdouble
# float64 has 2^-52; the reference has to be far below it (x87 80-bit: 2^-63 = 1.08e-19).  Where longdouble is
# float64 (or double-double with its looser guarantees) the dependent tests skip with REASON.
HAVE_EXTENDED = bool(np.finfo(LD).eps < 2e-19)
REASON = "numpy.longdouble has eps %.1e here, the reference needs < 2e-19" % float(np.finfo(LD).eps)


def chol_ld(A):
    """lower Cholesky factor of an SPD longdouble matrix, column by column (np.linalg does not take longdouble)"""
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        c = A[j:, j] - L[j:, :j] @ L[j, :j]
        assert c[0] > 0, ("not positive definite at column", j, float(c[0]))
        L[j, j] = np.sqrt(c[0])
        L[j + 1:, j] = c[1:] / L[j, j]
    return L


def fwd_ld(L, B):
    """L^-1 B for lower-triangular L by forward substitution, B a vector or a matrix of right-hand sides"""
    L = np.asarray(L, dtype=LD)
    X = np.array(B, dtype=LD)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def ekf_update_ref(P, idx, H, res, sigma2, form=None):
    """(P_plus, dx) in longdouble.  form None: the direct form for m <= n and the Gram form for m > n (the
    split the estimator makes); "direct" / "gram" force one of them (any m, n)."""
    P = np.asarray(P, dtype=LD)
    H = np.asarray(H, dtype=LD)
    res = np.asarray(res, dtype=LD)
    idx = np.asarray(idx, dtype=np.intp)
    s2 = LD(sigma2)
    m, n = H.shape
    assert idx.shape == (n,) and res.shape == (m,) and P.shape[0] == P.shape[1]
    if form is None:
        form = "direct" if m <= n else "gram"
    PI = P[idx, :]  # n x N, = P[:, I]^T
    if form == "direct":
        T = H @ PI  # m x N
        S = T[:, idx] @ H.T
        S = (S + S.T) / 2 + s2 * np.eye(m, dtype=LD)
        L = chol_ld(S)
        Wt = fwd_ld(L, T)  # W^T = L^-1 H P[I, :]
        return P - Wt.T @ Wt, Wt.T @ fwd_ld(L, res)
    assert form == "gram"
    L = chol_ld(PI[:, idx])
    Z = L.T @ (H.T @ H) @ L
    Z = (Z + Z.T) / 2 + s2 * np.eye(n, dtype=LD)
    U = chol_ld(Z)
    Vt = fwd_ld(L, PI)  # V^T = L^-1 P[I, :]
    Xt = fwd_ld(U, Vt)  # X^T = U^-1 V^T
    return P - Vt.T @ Vt + s2 * (Xt.T @ Xt), Xt.T @ fwd_ld(U, L.T @ (H.T @ res))


def gram_ref(A):
    A = np.asarray(A, dtype=LD)
    return A.T @ A


def scaled_err(A, B, P0):
    """max_ij |A_ij - B_ij| / sqrt(P0_ii P0_jj): the error in units of the prior correlation"""
    d = np.sqrt(np.diag(np.asarray(P0, dtype=LD)))
    return float(np.max(np.abs(np.asarray(A, dtype=LD) - np.asarray(B, dtype=LD)) / np.outer(d, d)))


def scaled_dx_err(a, b, P0):
    """max_i |a_i - b_i| / sqrt(P0_ii)"""
    d = np.sqrt(np.diag(np.asarray(P0, dtype=LD)))
    return float(np.max(np.abs(np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD)) / d))


def max_rel(a, b):
    """the suite's existing metric: max|a - b| / max|b|"""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), LD(1e-300)))


Case = namedtuple("Case", "P idx H res sigma2")


def graded_case(N, n, m, seed, sigma2, null=0, full=False):
    """A float64 update problem whose covariance spans eight orders of magnitude:
    P = D (A A^T / N + 1e-3 I) D with D a random permutation of logspace(-4, 0, N) (exactly symmetric);
    idx a random unsorted subset of n states (full: a random permutation of all N = n);
    H = randn(m, n) / D[idx], every row scaled by uniform(0.1, 1), so H P_II H^T is of order one whatever the
    scale of the states it touches; with null > 0 the unscaled H is first projected off `null` orthonormal
    directions q (H then annihilates D[idx] * q: exactly rank deficient, as an MSCKF stack is in its gauge
    directions); res = randn(m)."""
    rng = np.random.default_rng(seed)
    D = np.logspace(-4, 0, N)[rng.permutation(N)]
    A = rng.standard_normal((N, N))
    C = A @ A.T / N + 1e-3 * np.eye(N)
    P = C * np.outer(D, D)
    P = np.triu(P) + np.triu(P, 1).T
    if full:
        assert n == N
        idx = rng.permutation(N).astype(np.int32)
    else:
        idx = rng.choice(N, n, replace=False).astype(np.int32)
    H = rng.standard_normal((m, n))
    if null:
        Qn, _ = np.linalg.qr(rng.standard_normal((n, null)))
        H = H - (H @ Qn) @ Qn.T
    H = H / D[idx][None, :] * rng.uniform(0.1, 1.0, m)[:, None]
    res = rng.standard_normal(m)
    return Case(P, idx, np.ascontiguousarray(H), res, float(sigma2))


def case_id(c):
    return "-".join("%s%g" % (k, v) for k, v in c.items() if k != "seed" and v not in (0, False))


def _cases():
    direct, info = [], []
    seed = 1000
    sig = (2.25, 1e-2)
    # direct update: r over every panel_waves(r + 1) boundary and both sides of the LDS / global factor switch
    shapes = [(41, 24, r) for r in (1, 15, 16, 17, 63, 64, 111, 112, 137, 138, 159, 160, 207, 208, 255)]
    shapes += [(15, 15, 1), (16, 16, 16), (17, 1, 1), (33, 32, 40), (272, 255, 255)]
    for N, n, r in shapes:
        for s2 in sig:
            seed += 1
            direct.append(dict(N=N, n=n, m=r, seed=seed, sigma2=s2, null=0, full=(n == N)))
    # information form: rows n and n + 1 over every panel_waves boundary and both sides of each storage mode
    for n in (1, 15, 16, 17, 63, 64, 65, 111, 112, 113, 137, 138, 139, 159, 160, 161, 194, 195, 196, 207, 208, 209,
              254, 255):
        for s2 in sig:
            seed += 1
            info.append(dict(N=n + 9, n=n, m=n + 1, seed=seed, sigma2=s2, null=0, full=False))
    for n in (100, 139, 196, 243):
        for s2 in sig:
            seed += 1
            info.append(dict(N=n + 9, n=n, m=n + 37, seed=seed, sigma2=s2, null=4, full=False))
    for n in (64, 139, 196, 254):
        for s2 in sig:
            seed += 1
            info.append(dict(N=n, n=n, m=n + 1, seed=seed, sigma2=s2, null=0, full=True))
    # m == n takes the direct path and m == n + 1 the information path of the compressed entry
    edge = [dict(N=49, n=40, m=40, seed=1901, sigma2=2.25, null=0, full=False),
            dict(N=49, n=40, m=41, seed=1902, sigma2=2.25, null=0, full=False)]
    return direct, info, edge


DIRECT_CASES, INFO_CASES, EDGE_CASES = _cases()
# (m, ncol) of the compression: both Gram chunk sizes, the matrix-core Gram's threshold with a partial last slab,
# a second 64-column tile, and the reduce + Cholesky kernel's global-buffer path (ncol >= 139)
GRAM_CASES = [(2048, 9), (2049, 9), (8191, 9), (8192, 9), (8192 + 8, 70), (300, 139), (300, 150)]


def numeric_case(m, N=20, n=12):
    """An update whose result has a negative diagonal entry: P SPD except that P[0, 0] is 0 while row 0 keeps its
    correlations with the measured states idx (none of them state 0, so P_II is SPD and both forms run).  The
    update subtracts |W[0, :]|^2 > 0 from P[0, 0] = 0."""
    rng = np.random.default_rng(300 + m)
    A = rng.standard_normal((N, N))
    P = A @ A.T / N + 1e-3 * np.eye(N)
    P = np.triu(P) + np.triu(P, 1).T
    P[0, 0] = 0.0
    idx = (1 + rng.choice(N - 1, n, replace=False)).astype(np.int32)
    return Case(P, idx, rng.standard_normal((m, n)), rng.standard_normal(m), 1.0)


def gram_case(m, ncol):
    """full column rank, columns graded over two orders of magnitude"""
    rng = np.random.default_rng(7 * m + ncol)
    return rng.standard_normal((m, ncol)) * np.logspace(0, 2, ncol)[None, :]
