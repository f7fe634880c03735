"""Every size-dependent path of the device's EKF update family against the extended-precision reference
(tests/ekf_ref.py), one device call per case.

What the sizes reach (kernels_ekf.hip, kernels_cov.hip):
  * direct update, r rows: k_ekf_fact<W, LDS> with W = panel_waves(r + 1) = 1 (r <= 63), 2 (<= 111), 3 (<= 159),
    4 (<= 207), 5 (<= 255); the factor in LDS up to r = 137 and in global memory from 138.  N = 41 leaves a partial
    last 16-row tile of P; n == N, N = 15 / 16 / 17 and n = 1 are the small edges; (272, 255, 255) the largest.
  * information form, n columns (m = n + 1 rows, N = n + 9): k_info_cholP<W, mode> on n rows and k_info_cholZ<W, mode>
    on n + 1 rows; mode 0 (square in LDS) up to n = 138 (P) / 137 (Z), mode 1 (packed) up to 195 / 194, beyond that
    the four-launch split (k_info_split1 / _schur / split3 / _out) with its first block running from 176 columns
    down to 80.  n = 15 .. 17, 63 .. 65, 111 .. 113, 159 .. 161, 207 .. 209 are the panel-wave boundaries of both factors,
    137 .. 139 and 194 .. 196 both sides of each storage mode.  null = 4: H exactly rank deficient (m = n + 37).
    N == n: every state measured, the split's (n + 1) x (n | 1) work matrix is one row taller than P.
  * compression: k_gram with 64-row chunks (m <= 2048) and 512-row chunks, k_gram_mfma from 8192 rows (8200: a partial
    last slab and a second 64-column tile), k_gram_reduce_chol in LDS and, from 139 columns, in its global buffer.

Every update case asserts: P exactly symmetric; the suite's max-norm bounds against the oracle (1e-10 direct, 1e-9
compressed); and, in the metric that sees small-variance blocks (ekf_ref.scaled_err: |dP_ij| / sqrt(P_ii P_jj)),
    e_dev <= RATIO * max(e_orc, 16 * 2^-52)
for P and for dx, e_orc the oracle's own error against the same reference in the same test.  The inputs are graded
over eight orders of magnitude (ekf_ref.graded_case) and sigma2 is 2.25 or 1e-2.

RATIO = 64: 4 x the worst measured ratio, rounded up to a power of two.  Measured on MI355X over the 106 update cases:
    dx   15.0  information form N72-n63-m64-sigma20.01   (device 7.1e-13, oracle 4.8e-14)
    P+    4.30 information form N25-n16-m17-sigma20.01   (device 1.7e-14, oracle 3.9e-15)
The device sums its MFMA chains in another order than the oracle and multiplies by explicit inverses of the factors'
diagonal blocks where the oracle solves, so a small constant over the oracle is expected; at sigma2 = 2.25 no ratio
exceeds 2.2 and no device error 1e-14.  Largest device errors: P+ 4.1e-14 (N217-n208-m209-sigma20.01, oracle 9.8e-14),
dx 2.2e-12 (N264-n255-m256-sigma20.01, oracle 5.0e-13).  Compression: R^T R within 7.2e-16 of the extended Gram.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ekf_ref as R  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.HAVE_EXTENDED, reason=R.REASON)]

RATIO = 64.0
FLOOR = 16 * 2.0 ** -52


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def _update_case(c, compressed):
    import uvio_amd as U
    from oracle import oracle as O
    k = R.graded_case(**c)
    Pg, dxg = U.ekf_update(k.P, k.idx, k.H, k.res, k.sigma2, compressed=compressed)
    Po, dxo = O.ekf_update(k.P, k.idx, k.H, k.res, k.sigma2, compressed=compressed)
    Pr, dxr = R.ekf_update_ref(*k)
    e_dev, e_orc = R.scaled_err(Pg, Pr, k.P), R.scaled_err(Po, Pr, k.P)
    x_dev, x_orc = R.scaled_dx_err(dxg, dxr, k.P), R.scaled_dx_err(dxo, dxr, k.P)
    mP, mx = _rel(Pg, Po), _rel(dxg, dxo)
    print("EKFPATH %s P dev %.3e orc %.3e ratio %.2f dx dev %.3e orc %.3e ratio %.2f maxnorm %.1e %.1e" %
          (R.case_id(c), e_dev, e_orc, e_dev / max(e_orc, FLOOR), x_dev, x_orc, x_dev / max(x_orc, FLOOR), mP, mx))
    assert np.array_equal(Pg, Pg.T)
    tol = 1e-9 if compressed else 1e-10
    assert mP < tol and mx < tol, (mP, mx)
    assert e_dev <= RATIO * max(e_orc, FLOOR), (e_dev, e_orc)
    assert x_dev <= RATIO * max(x_orc, FLOOR), (x_dev, x_orc)


@pytest.mark.parametrize("c", R.DIRECT_CASES, ids=R.case_id)
def test_direct_update(c):
    _update_case(c, False)


@pytest.mark.parametrize("c", R.INFO_CASES, ids=R.case_id)
def test_information_form(c):
    assert c["m"] > c["n"]
    _update_case(c, True)


@pytest.mark.parametrize("c", R.EDGE_CASES, ids=R.case_id)
def test_compressed_entry_both_sides_of_m_equal_n(c):
    """m == n: the compressed entry runs the direct update; m == n + 1: the information form"""
    _update_case(c, True)


@pytest.mark.parametrize("m,ncol", R.GRAM_CASES)
def test_compress(m, ncol):
    import uvio_amd as U
    from oracle import oracle as O
    A = R.gram_case(m, ncol)
    Rg = U.compress(A)
    Ro = O.compress(A)
    assert np.array_equal(Rg, np.triu(Rg)) and np.all(np.diag(Rg) != 0)
    s = np.sign(np.diag(Rg)) * np.sign(np.diag(Ro))
    e_rows = _rel(Rg * s[:, None], Ro)
    G = R.gram_ref(A)
    e_dev, e_orc = R.max_rel(R.gram_ref(Rg), G), R.max_rel(R.gram_ref(Ro), G)
    print("GRAMPATH %d x %d R^T R dev %.3e orc %.3e rows %.1e" % (m, ncol, e_dev, e_orc, e_rows))
    assert e_rows < 1e-9, e_rows
    assert e_dev < 1e-12, e_dev


def _raises(name, *args, **kw):
    import uvio_amd as U
    with pytest.raises(RuntimeError, match=name):
        U.ekf_update(*args, **kw)


def test_capacity_limits():
    """More rows (direct) or columns (information form) than the 256-row factor panel holds, and more columns than
    the direct update's LDS staging holds: E_CAPACITY, before anything runs."""
    rng = np.random.default_rng(1)
    P = np.eye(300)
    idx = np.arange(40, dtype=np.int32)
    _raises("E_CAPACITY", P, idx, rng.standard_normal((256, 40)), np.zeros(256), 1.0)
    idx = np.arange(256, dtype=np.int32)
    _raises("E_CAPACITY", P, idx, rng.standard_normal((257, 256)), np.zeros(257), 1.0, compressed=True)
    Pw = np.eye(1216)
    _raises("E_CAPACITY", Pw, np.arange(1216, dtype=np.int32), rng.standard_normal((2, 1216)), np.zeros(2), 1.0)


@pytest.mark.parametrize("m,compressed", [(6, False), (13, True)])
def test_negative_diagonal_is_numeric_error(m, compressed):
    """tests/test_ekf_ref.py::test_negative_diagonal_input shows that this input drives P+[0, 0] below zero.  The
    reference exits there, so only the return code is compared."""
    k = R.numeric_case(m)
    assert (m > k.H.shape[1]) == compressed
    _raises("E_NUMERIC", k.P, k.idx, k.H, k.res, k.sigma2, compressed=compressed)


@pytest.mark.parametrize("n,m,compressed", [(24, 16, False), (24, 25, True), (200, 201, True)])
def test_zero_rows_change_nothing(n, m, compressed):
    """H = 0 and res = 0: P bit-identical and dx == 0.  The information form subtracts V V^T - sigma2 X X^T with
    X = V / sqrt(sigma2); sigma2 = 4 makes that scaling exact, so the two products cancel to the bit as well."""
    import uvio_amd as U
    k = R.graded_case(n + 9, n, m, 5, 4.0)
    Pg, dxg = U.ekf_update(k.P, k.idx, np.zeros((m, n)), np.zeros(m), k.sigma2, compressed=compressed)
    assert np.array_equal(Pg, k.P)
    assert np.all(dxg == 0.0)
