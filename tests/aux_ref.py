"""Caller-defined ("auxiliary") state variables restated in NumPy for tests/test_aux_ref.py and
tests/test_gpu_aux_state.py.  NumPy only: nothing from oracle/ or uvio_amd/.

A d-wide variable appended to an N x N covariance P:

  append (StateHelper::set_initial_covariance of the variable alone): zeros against [0, N), the prior's upper triangle
      mirrored into the new block
  init   (StateHelper::initialize_invertible, StateHelper.cpp:484-577), with I the measured columns:
      Ma = P[:, I] H_x^T,  cross = -Ma H_aux^-T,  M = H_x Ma[I] + R (upper triangle, mirrored),
      own = H_aux^-1 M H_aux^-T,  value = val0 + H_aux^-1 res
  walk   P[i][i] += sigma2 * dt

*_ref: numpy.longdouble, the reference (ekf_ref.HAVE_EXTENDED says whether longdouble is good for that here).
*_replay64: float64 in the device kernels' summation order (uvio_amd/csrc/kernels_cov.hip, k_aux_init /
k_aux_init_own / k_aux_walk), every product and every sum rounded by itself: the comparator whose own error against
the reference scales the device's bound, and for append and walk the expected bits.
"""
import hashlib

import numpy as np

import ekf_ref as E

LD = E.LD


def sym_upper(A, dtype=None):
    """the symmetric matrix whose upper triangle is A's; the strictly lower triangle of A is never read"""
    U = np.triu(np.asarray(A, dtype=dtype))
    return U + np.triu(U, 1).T


def append_ref(P, prior, dtype=np.float64):
    P = np.asarray(P, dtype=dtype)
    N, d = P.shape[0], np.shape(prior)[0]
    out = np.zeros((N + d, N + d), dtype=dtype)
    out[:N, :N] = P
    out[N:, N:] = sym_upper(np.asarray(prior)[:, :d], dtype)
    return out


def init_ref(P, idx, Hx, Hinv, R, dtype=LD):
    """the (N + d, N + d) covariance after initialize_invertible, in `dtype` arithmetic with NumPy's own sums"""
    P = np.asarray(P, dtype=dtype)
    Hx = np.asarray(Hx, dtype=dtype)
    Hinv = np.asarray(Hinv, dtype=dtype)
    idx = np.asarray(idx, dtype=np.intp)
    N, d = P.shape[0], Hinv.shape[0]
    Ma = P[:, idx] @ Hx.T if idx.size else np.zeros((N, d), dtype=dtype)
    M = (Hx @ Ma[idx, :] if idx.size else np.zeros((d, d), dtype=dtype)) + np.triu(np.asarray(R, dtype=dtype)[:, :d])
    M = sym_upper(M)
    out = np.zeros((N + d, N + d), dtype=dtype)
    out[:N, :N] = P
    out[:N, N:] = -Ma @ Hinv.T
    out[N:, :N] = out[:N, N:].T
    out[N:, N:] = sym_upper(Hinv @ M @ Hinv.T)
    return out


def lane_sum(prod):
    """The kernels' sum over the last axis: lane l of a 64-lane wavefront adds its terms k = l, l + 64, .. in
    ascending k to a partial that starts at 0.0; the 64 partials are then combined by six exchange steps
    v <- v + v[lane ^ o], o = 32, 16, 8, 4, 2, 1 (every lane ends with the same value)."""
    prod = np.asarray(prod, dtype=np.float64)
    n = prod.shape[-1]
    c = max((n + 63) // 64, 1)
    pad = np.zeros(prod.shape[:-1] + (64 * c,))
    pad[..., :n] = prod
    acc = np.zeros(prod.shape[:-1] + (64,))
    for j in range(c):
        acc = acc + pad[..., 64 * j:64 * j + 64]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lanes ^ o]
    return acc[..., 0]


def init_replay64(P, idx, Hx, Hinv, R):
    """init_ref in float64 with k_aux_init's and k_aux_init_own's summation order"""
    P = np.asarray(P, dtype=np.float64)
    Hx = np.asarray(Hx, dtype=np.float64)
    Hinv = np.asarray(Hinv, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.intp)
    N, d = P.shape[0], Hinv.shape[0]
    PI = P[:, idx]
    Ma = np.stack([lane_sum(PI * Hx[b][None, :]) for b in range(d)], axis=1) if N else np.zeros((0, d))
    out = np.zeros((N + d, N + d))
    out[:N, :N] = P
    for a in range(d):
        x = np.zeros(N)
        for b in range(d):
            x = x + Ma[:, b] * Hinv[a, b]
        out[:N, N + a] = 0.0 - x
        out[N + a, :N] = 0.0 - x
    M = np.zeros((d, d))
    for a in range(d):
        for b in range(a, d):
            M[a, b] = M[b, a] = lane_sum(Hx[a] * Ma[idx, b]) + R[a, b]
    U = np.zeros((d, d))
    for c in range(d):
        for b in range(d):
            s = 0.0
            for e in range(d):
                s = s + M[c, e] * Hinv[b, e]
            U[c, b] = s
    for a in range(d):
        for b in range(a, d):
            s = 0.0
            for c in range(d):
                s = s + Hinv[a, c] * U[c, b]
            out[N + a, N + b] = out[N + b, N + a] = s
    return out


def walk_replay64(P, cidx, sigma2, dt):
    """P[i][i] + fl(sigma2 * dt) in float64: the product rounded, then the sum"""
    out = np.array(P, dtype=np.float64)
    cidx = np.asarray(cidx, dtype=np.intp)
    step = np.asarray(sigma2, dtype=np.float64) * np.float64(dt)
    out[cidx, cidx] = out[cidx, cidx] + step
    return out


def walk_ref(P, cidx, sigma2, dt):
    out = np.array(P, dtype=LD)
    cidx = np.asarray(cidx, dtype=np.intp)
    out[cidx, cidx] += np.asarray(sigma2, dtype=LD) * LD(dt)
    return out


def scaled_err_new(A, B):
    """ekf_ref.scaled_err in the units of the augmented covariance B (the reference): max |A_ij - B_ij| /
    sqrt(B_ii B_jj).  The prior P has no diagonal for the new variable, so the reference's own is the scale."""
    B = np.asarray(B, dtype=LD)
    return E.scaled_err(A, B, B)


def digest(A):
    return hashlib.sha256(np.ascontiguousarray(A, dtype=np.float64).tobytes()).hexdigest()


def spd_case(N, seed):
    """ekf_ref.graded_case's covariance: SPD, exactly symmetric, variances over eight orders of magnitude"""
    rng = np.random.default_rng(seed)
    D = np.logspace(-4, 0, N)[rng.permutation(N)]
    A = rng.standard_normal((N, N))
    P = (A @ A.T / N + 1e-3 * np.eye(N)) * np.outer(D, D)
    return np.triu(P) + np.triu(P, 1).T, D


def init_case(N, d, n, seed):
    """P (spd_case), an unsorted non-contiguous column list (distinct while n <= N), H_x of order one in the units
    of the states it touches, a well-conditioned dense H_aux (its inverse formed in longdouble and rounded), and a
    dense SPD R graded over two orders of magnitude.  Returns (P, idx, Hx, Haux, Hinv, R)."""
    P, D = spd_case(N, seed)
    rng = np.random.default_rng(seed + 1)
    idx = rng.choice(N, n, replace=n > N).astype(np.int32)
    Hx = rng.standard_normal((d, n)) / D[idx][None, :] * rng.uniform(0.1, 1.0, d)[:, None]
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    Haux = Q * rng.uniform(0.5, 2.0, d)[None, :] + 0.05 * rng.standard_normal((d, d))
    Hinv = inverse_ld(Haux).astype(np.float64)
    Dr = np.logspace(-1, 0, d)[rng.permutation(d)]
    B = rng.standard_normal((d, d))
    R = sym_upper((B @ B.T / d + 1e-2 * np.eye(d)) * np.outer(Dr, Dr))
    return P, idx, np.ascontiguousarray(Hx), Haux, Hinv, R


def inverse_ld(A):
    """A^-1 in longdouble (Gauss-Jordan, partial pivoting); np.linalg does not take longdouble"""
    A = np.array(A, dtype=LD)
    d = A.shape[0]
    inv = np.eye(d, dtype=LD)
    for c in range(d):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        A[[c, p]], inv[[c, p]] = A[[p, c]], inv[[p, c]]
        piv = A[c, c]
        A[c], inv[c] = A[c] / piv, inv[c] / piv
        for i in range(d):
            if i != c:
                f = A[i, c]
                A[i], inv[i] = A[i] - f * A[c], inv[i] - f * inv[c]
    return inv
