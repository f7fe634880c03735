"""The pose-fix and quaternion-variable part of the C++ facade (include/uvio_hp.hpp): feed_pose, pose_results and
add_quat_state compile with g++ -Wall -Wextra -Werror and link against libuvio_hp.so, and construction without a GPU
throws uvio_amd::Error with UVIO_HP_E_DEVICE (tests/cpp/facade_pose_check.cpp).  The run on the device is
tests/test_gpu_pose_feed.py's facade test."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "euroc_mav", "estimator_config.yaml")


def build_check(tmp_path):
    lib = os.path.join(ROOT, "uvio_amd", "libuvio_hp.so")
    if not os.path.exists(lib):
        from uvio_amd import build
        build.build_product()
    exe = str(tmp_path / "facade_pose_check")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "facade_pose_check.cpp"), "-o", exe, lib,
           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def run_env():
    return dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))


def test_cpp_facade_pose_compiles_links_and_fails_loudly_without_gpu(tmp_path):
    import torch
    exe = build_check(tmp_path)
    env = run_env()
    if torch.cuda.is_available():
        env["HIP_VISIBLE_DEVICES"] = "-1"  # the program ends on the no-device construction error
    r = subprocess.run([exe, CFG, "nogpu"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "code -3" in r.stdout
