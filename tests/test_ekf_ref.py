"""tests/ekf_ref.py (the extended-precision EKF update that tests/test_gpu_ekf_paths.py compares the device
against) checked against itself, and the CPU oracle measured against it, on the exact case list of the GPU sweep.
CPU only.

  * The reference's two algebraic forms (direct: factor S; Gram: factor P_II and Z) are different computations of the
    same P+, dx and are run on the full H whatever m is.  P+ must agree within 1e-16 in scaled_err (worst measured
    5.8e-17, N41-n24-m15-sigma20.01).  dx within 1e-14 in scaled_dx_err: dx is the worse conditioned output (the
    float64 oracle errs by up to 6.6e-12 on these inputs, 3e4 * 2^-52, below), and the same conditioning at
    longdouble's 2^-64 is 3.2e-15, of which 1e-14 is three times.  Worst measured 2.2e-15
    (N252-n243-m280-sigma20.01-null4; there and wherever m > n it is the direct form that is off, it solves with S
    whose inverse carries res / sigma2 outside the range of H before P H^T cancels it: at
    N109-n100-m137-sigma20.01-null4 the Gram form is 1.9e-16 off a 45-digit solve and the direct form 1.1e-15).
    A slip in either form is an error of order one.
  * P+ is symmetric and P - P+ positive semi-definite.
  * The oracle (oracle/: the reference project's Eigen orderings in float64) stays under a cap in scaled_err,
    scaled_dx_err and, for its compression, in max|R^T R - A^T A| / max|A^T A| against the extended Gram.  This is
    the condition that the inputs are ones on which a correct float64 implementation is accurate: the device is
    then held to a small multiple of the oracle's error (test_gpu_ekf_paths.py).

The oracle measured on x86-64 (80-bit longdouble), worst over the case list; each cap is 8 x the worst:
    P+      2.92e-12  N41-n24-m255-sigma20.01       (sigma2 = 2.25: at most 1.1e-14, N41-n24-m255)
    dx      6.55e-12  N41-n24-m207-sigma20.01       (sigma2 = 2.25: at most 9.6e-15, N272-n255-m255)
    Gram    1.03e-14  8191 x 9
The large ones are the direct updates with many more rows than columns at sigma2 = 1e-2, where S = H P_II H^T +
sigma2 I has n eigenvalues of order m and m - n equal to sigma2.  A case above 1e-11 (ILL_CONDITIONED, asserted
beside the caps and below the P+ and dx caps) would be too ill-conditioned to discriminate: the input is to change
then, not the cap.

Sensitivity of the metric (test_scaled_metric_sees_a_small_block): the diagonal entry of the smallest prior variance
of the oracle's P+ moved by 1e-3 relative is an error of 5.8e-4 in scaled_err (the posterior variance is 0.58 of the
prior there) against a device bound of 2.3e-13 on that case, and of 1.1e-11 in max|dP| / max|P|, under the suite's
1e-10 max-norm bound.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ekf_ref as R  # noqa: E402

pytestmark = pytest.mark.skipif(not R.HAVE_EXTENDED, reason=R.REASON)

FORMS_TOL = 1e-16
FORMS_TOL_DX = 1e-14
ORACLE_CAP_P = 8 * 2.92e-12
ORACLE_CAP_DX = 8 * 6.55e-12
GRAM_CAP = 8 * 1.03e-14
ILL_CONDITIONED = 1e-11  # an oracle error above this: the input does not discriminate
ALL_CASES = R.DIRECT_CASES + R.INFO_CASES + R.EDGE_CASES


def _compressed(c):
    return c in R.INFO_CASES or c in R.EDGE_CASES


@pytest.mark.parametrize("c", ALL_CASES, ids=R.case_id)
def test_reference_and_oracle(c):
    from oracle import oracle as O
    k = R.graded_case(**c)
    Pr, dxr = R.ekf_update_ref(*k)
    assert Pr.dtype == np.longdouble and dxr.dtype == np.longdouble
    # the other algebraic form, on the full H
    if c["m"] <= 300:
        other = "gram" if c["m"] <= c["n"] else "direct"
        P2, dx2 = R.ekf_update_ref(*k, form=other)
        ef, efx = R.scaled_err(P2, Pr, k.P), R.scaled_dx_err(dx2, dxr, k.P)
        print("FORMS %s P %.2e dx %.2e" % (R.case_id(c), ef, efx))
        assert ef <= FORMS_TOL and efx <= FORMS_TOL_DX, (ef, efx)
    assert np.array_equal(Pr, Pr.T)
    w = np.linalg.eigvalsh((k.P - Pr).astype(np.float64))
    assert w[0] >= -1e-12 * np.abs(k.P).max(), w[0]
    Po, dxo = O.ekf_update(k.P, k.idx, k.H, k.res, k.sigma2, compressed=_compressed(c))
    eo, eox = R.scaled_err(Po, Pr, k.P), R.scaled_dx_err(dxo, dxr, k.P)
    print("ORACLE %s P %.2e dx %.2e" % (R.case_id(c), eo, eox))
    assert max(eo, eox) <= ILL_CONDITIONED, (eo, eox)
    assert eo <= ORACLE_CAP_P and eox <= ORACLE_CAP_DX, (eo, eox)


@pytest.mark.parametrize("m,ncol", R.GRAM_CASES)
def test_oracle_compress_against_extended_gram(m, ncol):
    from oracle import oracle as O
    A = R.gram_case(m, ncol)
    Ro = O.compress(A)
    e = R.max_rel(R.gram_ref(Ro), R.gram_ref(A))
    print("GRAM %d x %d %.2e" % (m, ncol, e))
    assert e <= min(GRAM_CAP, ILL_CONDITIONED), e


def test_direct_form_by_hand():
    """One state, one row: P = 4, H = 3, sigma2 = 13, res = 7: S = 49, K = 12 / 49, P+ = 4 - 144 / 49 = 52 / 49,
    dx = 84 / 49 = 12 / 7; the same from the Gram form (L = 2, Z = 36 + 13 = 49)."""
    LD = np.longdouble
    for form in ("direct", "gram"):
        Pp, dx = R.ekf_update_ref([[4.0]], [0], [[3.0]], [7.0], 13.0, form=form)
        assert abs(Pp[0, 0] - LD(52) / LD(49)) < 4e-19 and abs(dx[0] - LD(12) / LD(7)) < 4e-19


def test_metrics_by_hand():
    P0 = np.diag([1e-8, 1.0])
    B = np.array([[1e-8, 1e-5], [1e-5, 1.0]])
    A = B.copy()
    A[0, 0] *= 1 + 1e-3
    assert abs(R.scaled_err(A, B, P0) - 1e-3) < 1e-9
    assert abs(R.max_rel(A, B) - 1e-11) < 1e-17
    assert abs(R.scaled_dx_err([1e-4, 0.0], [0.0, 0.0], P0) - 1.0) < 1e-12


def test_scaled_metric_sees_a_small_block():
    """The gap this module closes: a 1e-3 relative error in the diagonal entry of the smallest prior variance of
    the oracle's P+ passes the suite's max-norm bound (1e-10) and fails the scaled bound by eight orders."""
    from oracle import oracle as O
    c = dict(N=41, n=24, m=16, seed=77, sigma2=2.25)
    k = R.graded_case(**c)
    Pr, _ = R.ekf_update_ref(*k)
    Po, _ = O.ekf_update(k.P, k.idx, k.H, k.res, k.sigma2)
    assert R.scaled_err(Po, Pr, k.P) <= ORACLE_CAP_P and R.max_rel(Po, Pr) < 1e-10
    i = int(np.argmin(np.diag(k.P)))
    Pb = Po.copy()
    Pb[i, i] *= 1 + 1e-3
    import test_gpu_ekf_paths as G
    bound = G.RATIO * max(R.scaled_err(Po, Pr, k.P), G.FLOOR)  # what the device is held to on this case
    print("SENSITIVITY max-norm %.2e scaled %.2e bound %.2e" % (R.max_rel(Pb, Pr), R.scaled_err(Pb, Pr, k.P), bound))
    assert R.max_rel(Pb, Pr) < 1e-10
    assert R.scaled_err(Pb, Pr, k.P) > 1e-4 > 1e6 * bound


def test_negative_diagonal_input():
    """The input of test_gpu_ekf_paths.py's E_NUMERIC case really drives P+[0, 0] below zero, in both forms."""
    for m in (6, 13):
        k = R.numeric_case(m)
        for form in ("direct", "gram"):
            Pp, _ = R.ekf_update_ref(*k, form=form)
            assert Pp[0, 0] < -1e-3 * k.P[1, 1], float(Pp[0, 0])
