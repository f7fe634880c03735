"""Buffered position fixes without a GPU: the NumPy model (tests/fix_ref.py) against central finite differences and
against the Python mirror's Jacobians, the float64 comparator against the longdouble reference, the library's exports,
and every refusal of uvio_hp_debug_position_update_p that needs no device.  The device's side is
tests/test_gpu_position_feed.py, the C++ facade's tests/test_facade_fix.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ekf_ref as E  # noqa: E402
import fix_ref as F  # noqa: E402
import meas_ref as M  # noqa: E402

needs_ld = pytest.mark.skipif(not E.HAVE_EXTENDED, reason=E.REASON)
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


def fd_fix_jacobian(q, p, s, Cm):
    """central differences of z over [dtheta (JPL left), dp, ds] in longdouble: step 1e-6, truncation O(step^2) =
    1e-12, rounding eps_ld / step = 1e-13 (tests/test_aux_ref.py's procedure)"""
    LD = E.LD
    q, p, s = np.asarray(q, dtype=LD), np.asarray(p, dtype=LD), np.asarray(s, dtype=LD)
    step = LD(1e-6)
    r = np.asarray(Cm).reshape(-1, 3).shape[0]
    J = np.zeros((r, 9), dtype=LD)
    for j in range(9):
        d = np.zeros(9, dtype=LD)
        d[j] = step
        hp = F.fix_h(M.quat_boxplus(q, d[:3]), p + d[3:6], s + d[6:], Cm)
        hm = F.fix_h(M.quat_boxplus(q, -d[:3]), p - d[3:6], s - d[6:], Cm)
        J[:, j] = (hp - hm) / (2 * step)
    return J


def random_fixes(seed=31):
    """(q, p, s, C) for r = 1, 2, 3, two random poses each; the altimeter and the identity among them"""
    rng = np.random.default_rng(seed)
    out = []
    for r in (1, 2, 3):
        for k in range(2):
            q = rng.standard_normal(4)
            Cm = rng.standard_normal((r, 3))
            if k == 1:
                Cm = {1: np.array([[0.0, 0.0, 1.0]]), 2: np.eye(3)[:2], 3: np.eye(3)}[r]
            out.append((q / np.linalg.norm(q), 5.0 * rng.standard_normal(3), rng.uniform(-1.0, 1.0, 3), Cm))
    return out


@needs_ld
@pytest.mark.parametrize("aux", [False, True], ids=["const", "aux"])
def test_model_matches_finite_differences(aux):
    for q, p, s, Cm in random_fixes():
        pred, H = F.fix_model(q, p, s, Cm, aux)
        r = Cm.shape[0]
        assert pred.shape == (r,) and H.shape == (r, 9 if aux else 6)
        assert np.max(np.abs(pred - Cm @ M.position_h(q, p, s))) < 1e-14
        J = fd_fix_jacobian(q, p, s, Cm)
        assert np.max(np.abs(H - J[:, :H.shape[1]])) < 1e-10


def test_model_is_the_python_mirrors_jacobian_under_C():
    from uvio_amd.manager import position_fix_jacobian, position_fix_lever_arm_jacobian
    for q, p, s, Cm in random_fixes(seed=32):
        h6, H6 = position_fix_jacobian(q, p, s)
        h9, H9 = position_fix_lever_arm_jacobian(q, p, s)
        for aux, h, H in ((False, h6, H6), (True, h9, H9)):
            pred, Hm = F.fix_model(q, p, s, Cm, aux, dtype=np.float64)
            assert np.max(np.abs(pred - Cm @ h)) < 1e-14 and np.max(np.abs(Hm - Cm @ H)) < 1e-14


@needs_ld
@pytest.mark.parametrize("r", [1, 2, 3])
@pytest.mark.parametrize("aux_id", [-1, 6, 14], ids=["const", "aux6", "auxN-3"])
def test_float64_comparator_against_the_reference(r, aux_id):
    k = F.fix_case(17, r, aux_id, seed=500 + 10 * r + aux_id)
    Pr, dxr, c_ref = F.fix_update_ref(k.P, k.imu_id, k.q, k.p, k.s, k.C, k.z, k.R, k.aux_id)
    P6, dx6, c_64 = F.fix_update_ref(k.P, k.imu_id, k.q, k.p, k.s, k.C, k.z, k.R, k.aux_id, dtype=np.float64)
    assert E.scaled_err(P6, Pr, k.P) < 1e-12 and E.scaled_dx_err(dx6, dxr, k.P) < 1e-12
    assert 0 < float(c_ref) < 100 and abs(float(c_64) - float(c_ref)) < 1e-10 * float(c_ref)
    # the triangle below R's diagonal is never read
    Rn = k.R + np.tril(np.full((r, r), np.nan), -1)
    Pn, dxn, cn = F.fix_update_ref(k.P, k.imu_id, k.q, k.p, k.s, k.C, k.z, Rn, k.aux_id)
    assert np.array_equal(Pn, Pr) and np.array_equal(dxn, dxr) and cn == c_ref


# ---- the library without a device ----
def test_library_exports_the_position_entries():
    from uvio_amd import _native as N
    lib = N.load()
    for name in ("feed_position", "get_position_results", "debug_position_update_p"):
        assert "uvio_hp_" + name in N.EXPORTED and hasattr(lib, "uvio_hp_" + name)
    q, n = C.c_int(-3), C.c_int(-3)
    one = np.ones(9)
    assert lib.uvio_hp_feed_position(None, 1.0, 3, one.ctypes.data_as(dp), one.ctypes.data_as(dp), one.ctypes.data_as(dp),
                                     3, one.ctypes.data_as(dp), 0, 1.0, C.byref(q)) == N.E_ARG
    assert lib.uvio_hp_get_position_results(None, None, None, None, 0, C.byref(n)) == N.E_ARG
    assert (q.value, n.value) == (-3, -3)


def _call_p(lib, k, **over):
    a = dict(P=np.array(k.P), N=k.P.shape[0], ld=k.P.shape[0], imu_id=k.imu_id, q=np.array(k.q), p=np.array(k.p),
             aux_id=k.aux_id, s=np.array(k.s), r=k.C.shape[0], C=np.array(k.C), z=np.array(k.z), R=np.array(k.R),
             ldr=k.R.shape[1], thr=float("inf"))
    a.update(over)
    P = a["P"].copy()
    dx = np.full(P.shape[0], 7.0)
    chi2, applied = C.c_double(-3.0), C.c_int(-3)

    def ptr(v):
        return None if v is None else v.ctypes.data_as(dp)

    rc = lib.uvio_hp_debug_position_update_p(ptr(P), a["N"], a["ld"], a["imu_id"], ptr(a["q"]), ptr(a["p"]), a["aux_id"],
                                             ptr(a["s"]), a["r"], ptr(a["C"]), ptr(a["z"]), ptr(a["R"]), a["ldr"],
                                             a["thr"], ptr(dx), C.byref(chi2), C.byref(applied))
    untouched = np.array_equal(P, a["P"]) and np.all(dx == 7.0) and (chi2.value, applied.value) == (-3.0, -3)
    return rc, untouched


def test_standalone_refusals_need_no_device():
    """every argument check of uvio_hp_debug_position_update_p comes before the device is touched"""
    from uvio_amd import _native as N
    lib = N.load()
    k = F.fix_case(17, 3, 14, seed=77)
    nan_z, nan_q, neg_R = np.array(k.z), np.array(k.q), np.array(k.R)
    nan_z[1] = np.nan
    nan_q[0] = np.inf
    neg_R[1, 1] = -neg_R[1, 1]
    bad = [dict(r=0), dict(r=4), dict(ldr=2), dict(ld=16), dict(N=5, ld=5), dict(imu_id=-1), dict(imu_id=12),
           dict(aux_id=15), dict(aux_id=5), dict(aux_id=3), dict(thr=0.0), dict(thr=-1.0), dict(thr=float("nan")),
           dict(z=nan_z), dict(q=nan_q), dict(R=neg_R), dict(q=None), dict(s=None), dict(C=None)]
    for over in bad:
        rc, untouched = _call_p(lib, k, **over)
        assert rc == N.E_ARG and untouched, over


def test_valid_standalone_call_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from uvio_amd import _native as N
    rc, untouched = _call_p(N.load(), F.fix_case(17, 3, 14, seed=77))
    assert rc == N.E_DEVICE and untouched
