"""The NumPy reference of the dense-R measurement update (tests/meas_ref.py) held against itself, the position-fix
Jacobian of the Python mirror and of the C++ facade against finite differences, and the library's four new exports.
No GPU: the device's side of these is tests/test_gpu_meas_update.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import ekf_ref as E  # noqa: E402
import meas_ref as M  # noqa: E402

needs_ld = pytest.mark.skipif(not E.HAVE_EXTENDED, reason=E.REASON)
# the shapes of the identities: one row, a partial tile, more rows than one tile
SMALL = [(15, 1, 1), (17, 6, 6), (41, 24, 17)]


@needs_ld
@pytest.mark.parametrize("s", SMALL, ids=M.shape_id)
def test_isotropic_R_is_the_sigma2_reference(s):
    """R = sigma2 I: the same (P+, dx) as ekf_ref.ekf_update_ref's direct form, operation for operation"""
    k = E.graded_case(s[0], s[1], s[2], M.shape_seed(s), 0.37)
    Pr, dxr = E.ekf_update_ref(k.P, k.idx, k.H, k.res, k.sigma2, form="direct")
    Pm, dxm, chi2 = M.ekf_update_R_ref(k.P, k.idx, k.H, k.res, k.sigma2 * np.eye(s[2]))
    assert E.scaled_err(Pm, Pr, k.P) < 1e-17 and E.scaled_dx_err(dxm, dxr, k.P) < 1e-17
    assert chi2 > 0


@needs_ld
@pytest.mark.parametrize("s", SMALL, ids=M.shape_id)
def test_whitening_identity(s):
    """(L_R^-1 H, L_R^-1 res, I) is the same measurement as (H, res, R = L_R L_R^T)"""
    k = M.graded_R_case(*s, seed=M.shape_seed(s))
    LR = E.chol_ld(k.R)
    Hw, rw = E.fwd_ld(LR, k.H), E.fwd_ld(LR, k.res)
    P1, dx1, c1 = M.ekf_update_R_ref(k.P, k.idx, k.H, k.res, k.R)
    P2, dx2, c2 = M.ekf_update_R_ref(k.P, k.idx, Hw, rw, np.eye(s[2]))
    # two routes in 64-bit-mantissa arithmetic (eps 1.1e-19) that differ by a solve with L_R: R = D C D with D^2
    # graded over 1e4 and cond(C) <= (4 + 1e-3) / 1e-3, so cond(R) <= 4e7 and the routes may differ by
    # r cond(R) eps = 17 * 4e7 * 1.1e-19 = 7e-11 in relative terms; 1e-10 is that bound, rounded up
    assert E.scaled_err(P1, P2, k.P) < 1e-10 and E.scaled_dx_err(dx1, dx2, k.P) < 1e-10
    assert abs(float(c1 - c2)) < 1e-10 * float(c1)


@pytest.mark.parametrize("dtype", [np.float64, E.LD], ids=["f64", "ld"])
def test_lower_triangle_of_R_is_never_read(dtype):
    s = (41, 24, 17)
    k = M.graded_R_case(*s, seed=M.shape_seed(s))
    Rg = np.triu(k.R) + np.tril(np.full_like(k.R, np.nan), -1)
    a = M.ekf_update_R_ref(k.P, k.idx, k.H, k.res, k.R, dtype)
    b = M.ekf_update_R_ref(k.P, k.idx, k.H, k.res, Rg, dtype)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y))


@needs_ld
@pytest.mark.parametrize("s", M.SHAPES, ids=M.shape_id)
def test_float64_comparator_chi2_within_the_gate_tests_bound(s):
    """tests/test_gpu_meas_update.py asks the device's chi2 to be within 1e-10 (relative) of the reference's; the
    float64 comparator has to meet that bound itself on the same cases"""
    k = M.graded_R_case(*s, seed=M.shape_seed(s))
    c_ld = M.ekf_update_R_ref(*k)[2]
    c_64 = M.ekf_update_R_ref(*k, dtype=np.float64)[2]
    assert abs(float(c_64 - c_ld)) < 1e-10 * float(c_ld), (float(c_64), float(c_ld))


# ---- position_fix's Jacobian ----
_POSES = [([0.1, -0.2, 0.3, 0.9], [1.0, -2.0, 0.5], [0.2, -0.1, 0.05]),
          ([-0.5, 0.5, 0.5, 0.5], [10.0, 3.0, -4.0], [0.0, 0.3, -0.7]),
          ([0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [1.0, 2.0, 3.0])]


def _fd_jacobian(q, p, s):
    """central differences of h over the IMU pose's error state [dtheta (JPL left), dp] in longdouble: step 1e-6,
    truncation O(step^2) = 1e-12, rounding eps_ld / step = 1e-13"""
    LD = E.LD
    q, p, s = np.asarray(q, dtype=LD), np.asarray(p, dtype=LD), np.asarray(s, dtype=LD)
    step = LD(1e-6)
    J = np.zeros((3, 6), dtype=LD)
    for j in range(6):
        d = np.zeros(6, dtype=LD)
        d[j] = step
        hp = M.position_h(M.quat_boxplus(q, d[:3]), p + d[3:], s)
        hm = M.position_h(M.quat_boxplus(q, -d[:3]), p - d[3:], s)
        J[:, j] = (hp - hm) / (2 * step)
    return J


@needs_ld
@pytest.mark.parametrize("q,p,s", _POSES)
def test_position_fix_jacobian_python_mirror_matches_finite_differences(q, p, s):
    from uvio_amd.manager import position_fix_jacobian
    q = np.asarray(q) / np.linalg.norm(q)
    h, H = position_fix_jacobian(q, p, s)
    assert np.max(np.abs(h - M.position_h(q, np.asarray(p), np.asarray(s)))) < 1e-14
    assert np.max(np.abs(H - _fd_jacobian(q, p, s))) < 1e-10


def _build_check(tmp_path):
    lib = os.path.join(ROOT, "uvio_amd", "libuvio_hp.so")
    if not os.path.exists(lib):
        from uvio_amd import build
        build.build_product()
    exe = str(tmp_path / "facade_meas_check")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "facade_meas_check.cpp"), "-o", exe, lib,
           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


@needs_ld
def test_position_fix_jacobian_header_matches_finite_differences(tmp_path):
    """include/uvio_hp.hpp's position_fix_jacobian, compiled with g++ -Werror as tests/test_facade.py compiles
    the facade, evaluated by tests/cpp/facade_meas_check.cpp"""
    import torch
    exe = _build_check(tmp_path)
    cfg = os.path.join(ROOT, "configs", "euroc_mav", "estimator_config.yaml")
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    if torch.cuda.is_available():
        env["HIP_VISIBLE_DEVICES"] = "-1"  # the program ends on the no-device construction error
    for q, p, s in _POSES:
        q = np.asarray(q) / np.linalg.norm(q)
        args = ["%.17g" % v for v in list(q) + list(p) + list(s)]
        r = subprocess.run([exe, cfg] + args, capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        v = np.array([float(x) for x in [ln for ln in r.stdout.splitlines() if ln.startswith("JAC")][0].split()[1:]])
        assert np.max(np.abs(v[:3] - M.position_h(q, np.asarray(p), np.asarray(s)))) < 1e-14
        assert np.max(np.abs(v[3:].reshape(3, 6) - _fd_jacobian(q, p, s))) < 1e-10


# ---- the library's side that needs no device ----
def test_library_exports_the_new_entries_and_chi2_95_matches_scipy():
    """uvio_hp_propagate, uvio_hp_measurement_update, uvio_hp_ekf_update_r and uvio_hp_chi2_95 are exported, and the
    table is scipy's chi2.ppf(0.95, dof) (tests/golden/chi2_095.json holds scipy's values; scipy itself is asked
    too where it is installed)"""
    from uvio_amd import _native as N
    import uvio_amd as U
    lib = N.load()
    for name in ("uvio_hp_propagate", "uvio_hp_measurement_update", "uvio_hp_ekf_update_r", "uvio_hp_chi2_95"):
        assert hasattr(lib, name) and name in N.EXPORTED, name
    g = json.load(open(os.path.join(HERE, "golden", "chi2_095.json")))["table"]
    for dof in (1, 3, 10, 999):
        assert abs(U.chi2_95(dof) - g[str(dof)]) < 1e-9 * g[str(dof)], dof
    try:
        from scipy.stats import chi2
    except ImportError:
        chi2 = None
    if chi2 is not None:
        for dof in (1, 3):
            assert abs(U.chi2_95(dof) - chi2.ppf(0.95, dof)) < 1e-9 * chi2.ppf(0.95, dof), dof
    out = C.c_double(-1.0)
    for dof in (0, -1, 1000):
        assert lib.uvio_hp_chi2_95(dof, C.byref(out)) == N.E_ARG and out.value == -1.0
    assert lib.uvio_hp_chi2_95(1, None) == N.E_ARG


def test_measurement_update_refusals_need_no_device():
    """every argument check of uvio_hp_ekf_update_r comes before the device is touched: they answer on a host
    without one, and leave the outputs alone"""
    import uvio_amd as U
    k = M.graded_R_case(17, 6, 6, seed=11)
    with pytest.raises(RuntimeError, match="E_CAPACITY"):
        U.ekf_update_R(np.eye(300), np.arange(40, dtype=np.int32), np.ones((256, 40)), np.zeros(256), np.eye(256))
    with pytest.raises(RuntimeError, match="E_ARG"):
        U.ekf_update_R(k.P, k.idx, k.H, k.res, k.R, ldr=5)
    bad = k.res.copy()
    bad[2] = np.nan
    with pytest.raises(RuntimeError, match="E_ARG"):
        U.ekf_update_R(k.P, k.idx, k.H, bad, k.R)
    for thr in (0.0, -1.0, float("nan")):
        with pytest.raises(RuntimeError, match="E_ARG"):
            U.ekf_update_R(k.P, k.idx, k.H, k.res, k.R, chi2_thr=thr)
    idx = k.idx.copy()
    idx[0] = 17
    with pytest.raises(RuntimeError, match="E_ARG"):
        U.ekf_update_R(k.P, idx, k.H, k.res, k.R)
    # a NaN below R's diagonal is not an argument error: that triangle is never read (the call then needs a device)
