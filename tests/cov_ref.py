"""The covariance bookkeeping kernels (uvio_amd/csrc/kernels_cov.hip: k_prop_T, k_prop_write, k_prop_clone, k_clone,
k_marginalize, k_marginalize_multi, k_compact, k_marginal_gather) restated in NumPy for tests/test_cov_ref.py and
tests/test_gpu_cov_ops.py.  NumPy only: nothing from oracle/ or uvio_amd/.

  propagate (StateHelper::EKFPropagation, StateHelper.cpp:36-114), I = iold, B = the new block's indices:
      T = P[:, I] Phi^T,  P[:, B] = T,  P[B, :] = T^T,  P[B, B] = Q (upper triangle, mirrored) + Phi T[I, :]
  clone (StateHelper::clone of the 6-wide IMU pose at src0 + augment_clone's time-offset term, :341-391, :579-616):
      C = [[P, P[:, S]], [P[S, :], P[S, S]]],  C[:, N:] += C[:, dt] dnc^T,  then C[N:, :] += dnc C[dt, :]
  marginalize (StateHelper::marginalize, :271-339): the kept rows / columns, the lower-left block copied from the
      transposed upper-right one

*_ref: numpy.longdouble with NumPy's own sums, the reference (ekf_ref.HAVE_EXTENDED says whether longdouble is good
for that here).  *_replay64: float64 in exactly the kernels' order, every product and every sum rounded by itself (the
library is built with -ffp-contract=off): the bits the device is expected to return.
"""
import itertools

import numpy as np

import ekf_ref as E

LD = E.LD
U53 = 2.0 ** -53  # float64's unit roundoff
NAN_FILL = np.array([0x7FF8C0DEC0DE0001], dtype=np.uint64).view(np.float64)[0]  # a quiet NaN that names itself


def same_bits(a, b):
    """the comparison of the GPU tests: the same shape and the same 64 bits in every entry (NaN payloads and the sign
    of a zero included)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def sym_upper(Q, dtype=None):
    """the symmetric matrix whose upper triangle is Q's; the strictly lower triangle of Q is never read"""
    Q = np.asarray(Q)
    out = np.zeros(Q.shape, dtype=dtype or Q.dtype)
    iu = np.triu_indices(Q.shape[0])
    out[iu] = Q[iu]
    out[(iu[1], iu[0])] = Q[iu]
    return out


# ---- propagation ----
def propagate_ref(P, new, iold, Phi, Q, dtype=LD):
    """EKFPropagation in `dtype`: `new` the block's covariance indices (p), iold the columns Phi (p, q) multiplies"""
    P = np.asarray(P, dtype=dtype)
    Phi = np.asarray(Phi, dtype=dtype)
    new, iold = np.asarray(new, dtype=np.intp), np.asarray(iold, dtype=np.intp)
    T = P[:, iold] @ Phi.T
    out = P.copy()
    out[:, new] = T
    out[new, :] = T.T
    out[np.ix_(new, new)] = sym_upper(Q, dtype) + Phi @ T[iold, :]
    return out


def propagate_T64(P, iold, Phi):
    """k_prop_T (and k_prop_clone's first phase): T[i][a] from 0.0 over ascending b, product and sum rounded"""
    P = np.asarray(P, dtype=np.float64)
    Phi = np.asarray(Phi, dtype=np.float64)
    T = np.zeros((P.shape[0], Phi.shape[0]))
    for b, col in enumerate(np.asarray(iold, dtype=np.intp)):
        T = T + P[:, col][:, None] * Phi[:, b][None, :]
    return T


def propagate_replay64(P, new, iold, Phi, Q):
    """k_prop_T then k_prop_write: a block entry starts from the mirrored upper Q and adds Phi[x][c] * T[iold[c]][a]
    over ascending c; every other row i stores T[i][a] at (i, new[a]) and (new[a], i)"""
    P = np.asarray(P, dtype=np.float64)
    Phi = np.asarray(Phi, dtype=np.float64)
    new, iold = np.asarray(new, dtype=np.intp), np.asarray(iold, dtype=np.intp)
    T = propagate_T64(P, iold, Phi)
    acc = sym_upper(np.asarray(Q, dtype=np.float64))
    for c, row in enumerate(iold):
        acc = acc + Phi[:, c][:, None] * T[row, :][None, :]
    out = P.copy()
    out[:, new] = T
    out[new, :] = T.T
    out[np.ix_(new, new)] = acc
    return out


def propagate_bound(P, new, iold, Phi, Q):
    """Entry-wise bound of |propagate_replay64 - propagate_ref| on the rows / columns of the block (zero elsewhere):
    a recursive sum of q rounded products has an error below q u (1 + q u) times the sum of the terms' magnitudes (u =
    2^-53), so a cross entry T[i][a] is within (q + 1) u (|P[i, I]| |Phi|^T)[a]; a block entry adds q more such
    terms and Q on top of the T it reads (2 q + 1 roundings in a chain): (2 q + 4) u (|Q| + |Phi| |P_II| |Phi|^T).
    The spare units cover the second-order terms and the longdouble reference's own 2^-64."""
    P = np.abs(np.asarray(P, dtype=LD))
    Phi = np.abs(np.asarray(Phi, dtype=LD))
    new, iold = np.asarray(new, dtype=np.intp), np.asarray(iold, dtype=np.intp)
    q = iold.size
    cross = (q + 1) * LD(U53) * (P[:, iold] @ Phi.T)
    out = np.zeros(P.shape, dtype=LD)
    out[:, new] = cross
    out[new, :] = cross.T
    out[np.ix_(new, new)] = (2 * q + 4) * LD(U53) * (np.abs(sym_upper(Q, LD)) + Phi @ P[np.ix_(iold, iold)] @ Phi.T)
    return out


# ---- clone ----
def clone_ref(P, src0, dt_id=-1, dnc=None, dtype=LD):
    """StateHelper::clone of the pose at src0 and augment_clone's two += statements, in `dtype`"""
    P = np.asarray(P, dtype=dtype)
    N = P.shape[0]
    S = slice(src0, src0 + 6)
    C = np.zeros((N + 6, N + 6), dtype=dtype)
    C[:N, :N] = P
    C[N:, N:] = P[S, S]
    C[:N, N:] = P[:, S]
    C[N:, :N] = P[S, :]
    if dt_id >= 0:
        d = np.asarray(dnc, dtype=dtype).reshape(6)
        C[:, N:] = C[:, N:] + np.outer(C[:, dt_id], d)
        C[N:, :] = C[N:, :] + np.outer(d, C[dt_id, :])
    return C


def clone_replay64(P, src0, dt_id=-1, dnc=None):
    """k_clone (and k_prop_clone's third phase), each expression in the kernel's order:
         col[i][b]   = P[i][S b] + P[i][dt] * d[b]          row[b][i] = P[S b][i] + d[b] * P[dt][i]
         block[a][b] = (P[S a][S b] + P[S a][dt] * d[b]) + d[a] * (P[dt][S b] + P[dt][dt] * d[b])"""
    P = np.asarray(P, dtype=np.float64)
    N = P.shape[0]
    S = slice(src0, src0 + 6)
    C = np.zeros((N + 6, N + 6))
    C[:N, :N] = P
    col, row, blk = P[:, S].copy(), P[S, :].copy(), P[S, S].copy()
    if dt_id >= 0:
        d = np.asarray(dnc, dtype=np.float64).reshape(6)
        col = col + P[:, dt_id][:, None] * d[None, :]
        row = row + d[:, None] * P[dt_id, :][None, :]
        blk = blk + P[S, dt_id][:, None] * d[None, :]
        blk = blk + d[:, None] * (P[dt_id, S][None, :] + P[dt_id, dt_id] * d[None, :])
    C[:N, N:], C[N:, :N], C[N:, N:] = col, row, blk
    return C


def clone_bound(P, src0, dt_id=-1, dnc=None):
    """Entry-wise bound of |clone_replay64 - clone_ref|: without the time-offset term the clone is a copy (zero).
    With it no quantity passes through more than four roundings (P[dt][dt] d[b]: the product, the inner sum, the
    product with d[a], the outer sum), so 5 u times the sum of the magnitudes of an entry's three kinds of terms --
    the copied entry, the single products with d, the double product -- bounds it, second order included."""
    Pa = np.abs(np.asarray(P, dtype=LD))
    N = Pa.shape[0]
    out = np.zeros((N + 6, N + 6), dtype=LD)
    if dt_id < 0:
        return out
    d = np.abs(np.asarray(dnc, dtype=LD).reshape(6))
    S = slice(src0, src0 + 6)
    k = 5 * LD(U53)
    out[:N, N:] = k * (Pa[:, S] + np.outer(Pa[:, dt_id], d))
    out[N:, :N] = k * (Pa[S, :] + np.outer(d, Pa[dt_id, :]))
    out[N:, N:] = k * (Pa[S, S] + np.outer(Pa[S, dt_id], d) + np.outer(d, Pa[dt_id, S]) + Pa[dt_id, dt_id] * np.outer(d, d))
    return out


def expected_buffer(P, new, iold, Phi, Q, clone_src=None, dt_id=-1, dnc=None, ld=None, fill=NAN_FILL):
    """what uvio_hp_debug_cov_propagate_p returns, padding included: the replay in the top-left corner of a buffer
    whose other entries keep `fill`"""
    out = propagate_replay64(P, new, iold, Phi, Q)
    if clone_src is not None:
        out = clone_replay64(out, clone_src, dt_id, dnc)
    n = out.shape[0]
    buf = np.full((n, n if ld is None else ld), fill, dtype=np.float64)
    buf[:, :n] = out
    return buf


# ---- marginalization and the gathers ----
def marginalize_one(P, m0, ms):
    """StateHelper::marginalize of [m0, m0 + ms): x1 = [0, m0), x2 = [m0 + ms, N); the lower-left block is the
    transposed upper-right one, never P's own lower-left"""
    P = np.asarray(P)
    N = P.shape[0]
    x2 = N - m0 - ms
    out = np.zeros((N - ms, N - ms), dtype=P.dtype)
    out[:m0, :m0] = P[:m0, :m0]
    out[:m0, m0:] = P[:m0, m0 + ms:]
    out[m0:, :m0] = out[:m0, m0:].T
    out[m0:, m0:] = P[m0 + ms:, m0 + ms:]
    assert out[m0:, m0:].shape == (x2, x2)
    return out


def marginalize_seq(P, variables, order=None):
    """marginalize_one for every (id, size) of `variables` (ids in P's own numbering, disjoint), in the sequence
    `order` (indices into variables; None: as listed), the ids of the later ones shifted as the state shrinks"""
    out = np.asarray(P)
    live = [list(v) for v in variables]
    for k in (range(len(live)) if order is None else order):
        m0, ms = live[k]
        out = marginalize_one(out, m0, ms)
        for v in live:
            if v[0] > m0:
                v[0] -= ms
    return out


def kept_indices(N, variables):
    gone = np.zeros(N, dtype=bool)
    for m0, ms in variables:
        gone[m0:m0 + ms] = True
    return np.flatnonzero(~gone).astype(np.int32)


def flip_mask(src):
    """k_marginalize_multi's rule: the lower entry (i > j) comes from the upper triangle exactly when more indices
    were removed before src[i] than before src[j]"""
    src = np.asarray(src, dtype=np.intp)
    k = np.arange(src.size)
    removed_before = src - k
    return (k[:, None] > k[None, :]) & (removed_before[:, None] > removed_before[None, :])


def marginalize_multi_model(P, src, rule="rule"):
    """k_marginalize_multi as written (rule), with its rule inverted or dropped (the injected errors of the tests)"""
    P = np.asarray(P)
    src = np.asarray(src, dtype=np.intp)
    direct, flipped = P[np.ix_(src, src)], P[np.ix_(src, src)].T
    f = flip_mask(src)
    if rule == "inverted":
        k = np.arange(src.size)
        f = (k[:, None] > k[None, :]) & ~f
    elif rule == "dropped":
        f = np.zeros_like(f)
    return np.where(f, flipped, direct)


def all_orders(n):
    return list(itertools.permutations(range(n)))


# ---- inputs ----
def coded(N, symmetric=False):
    """P[i][j] = 4096 i + j: every value exact and unique, so equality names the source element (symmetric: the
    upper triangle's codes mirrored)"""
    i, j = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    if symmetric:
        i, j = np.minimum(i, j), np.maximum(i, j)
    return (i * 4096 + j).astype(np.float64)


def cov_case(N, seed):
    """P = D (A A^T / N + 1e-3 I) D with D a permutation of logspace(-4, 1, N): variances graded from 1e-8 to 1e2.
    The strictly lower triangle is then moved by k ulp, k in {-3 .. 3} \\ {0} by position: P is symmetric only up to
    rounding, as the propagated IMU block is, and the triangle a kernel reads shows in the bits."""
    rng = np.random.default_rng(seed)
    D = np.logspace(-4, 1, N)[rng.permutation(N)] if N > 1 else np.array([1.0])
    A = rng.standard_normal((N, N))
    P = (A @ A.T / N + 1e-3 * np.eye(N)) * np.outer(D, D)
    P = np.triu(P) + np.triu(P, 1).T
    i, j = np.tril_indices(N, -1)
    k = (7 * i + 13 * j) % 7 - 3
    k[k == 0] = 2
    P[i, j] = P[i, j] * (1.0 + k * 2.0 ** -52)
    return P


def phi_case(new, iold, seed):
    """Phi (p, q) near the identity (1 + small where a row's own column is among iold), its other entries of mixed
    sign and of magnitudes from 1e-6 to 1"""
    rng = np.random.default_rng(seed)
    p, q = len(new), len(iold)
    Phi = rng.standard_normal((p, q)) * 10.0 ** rng.uniform(-6.0, 0.0, (p, q))
    for a, r in enumerate(new):
        for b, c in enumerate(iold):
            if r == c:
                Phi[a, b] = 1.0 + 1e-3 * rng.standard_normal()
    return np.ascontiguousarray(Phi)


def q_case(p, seed, zero=False):
    """a small SPD Q in the upper triangle, NaN below the diagonal: the kernels must never read it there"""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((p, p))
    Qs = (B @ B.T / p + 1e-2 * np.eye(p)) * 1e-6 * np.outer(np.logspace(-2, 0, p), np.logspace(-2, 0, p))
    if zero:
        Qs = np.zeros((p, p))
    return np.triu(Qs) + np.tril(np.full((p, p), np.nan), -1)


def iold_case(N, s0, p, q, seed):
    """q distinct columns for a block [s0, s0 + p): the block itself when q == p; the block plus other columns when
    q > p; a part of the block plus other columns when q < p -- shuffled, so no order is assumed"""
    rng = np.random.default_rng(seed)
    block = np.arange(s0, s0 + p)
    others = np.setdiff1d(np.arange(N), block)
    if q == p:
        return block.astype(np.int32)
    if q > p:
        cols = np.concatenate([block, rng.choice(others, q - p, replace=False)])
    else:
        keep = max(q - 2, 1)
        cols = np.concatenate([rng.choice(block, keep, replace=False), rng.choice(others, q - keep, replace=False)])
    return rng.permutation(cols).astype(np.int32)
