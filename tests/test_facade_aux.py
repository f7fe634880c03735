"""The aux-state part of the C++ facade (include/uvio_hp.hpp): add_state, add_state_from_measurement, aux_state,
remove_state, position_fix_lever_arm and position_fix_lever_arm_jacobian compile with g++ -Wall -Wextra -Werror and
link against libuvio_hp.so; the header's Jacobian is compared with central finite differences on random poses; and
construction without a GPU throws uvio_amd::Error with UVIO_HP_E_DEVICE (tests/cpp/facade_aux_check.cpp).  The run on
the device is tests/test_gpu_aux_state.py's facade test."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import ekf_ref as E  # noqa: E402

CFG = os.path.join(ROOT, "configs", "euroc_mav", "estimator_config.yaml")


def build_check(tmp_path):
    lib = os.path.join(ROOT, "uvio_amd", "libuvio_hp.so")
    if not os.path.exists(lib):
        from uvio_amd import build
        build.build_product()
    exe = str(tmp_path / "facade_aux_check")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "facade_aux_check.cpp"), "-o", exe, lib,
           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def run_env():
    return dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))


@pytest.mark.skipif(not E.HAVE_EXTENDED, reason=E.REASON)
def test_cpp_facade_aux_compiles_links_matches_finite_differences_and_fails_loudly_without_gpu(tmp_path):
    import torch
    from test_aux_ref import fd_lever_arm_jacobian, lever_arm_h, random_poses
    exe = build_check(tmp_path)
    env = run_env()
    if torch.cuda.is_available():
        env["HIP_VISIBLE_DEVICES"] = "-1"  # the program ends on the no-device construction error
    for q, p, arm in random_poses(3, seed=22):
        args = ["%.17g" % v for v in list(q) + list(p) + list(arm)]
        r = subprocess.run([exe, CFG, "jac"] + args, capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        v = np.array([float(x) for x in [ln for ln in r.stdout.splitlines() if ln.startswith("JACL")][0].split()[1:]])
        assert np.max(np.abs(v[:3] - lever_arm_h(q, p, arm))) < 1e-14
        assert np.max(np.abs(v[3:].reshape(3, 9) - fd_lever_arm_jacobian(q, p, arm))) < 1e-10
        assert "code -3" in r.stdout
