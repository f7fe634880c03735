"""The odometry part of the C++ facade (include/uvio_hp.hpp): marginal_covariance, good_features_MSCKF,
enable_odometry, fast_state_propagate and the ROS covariance reordering compile with g++ -Wall -Wextra -Werror,
link against libuvio_hp.so, the reordering matches ROS1Visualizer.cpp:311-325 on a 12 x 12 of distinct integers,
and construction without a GPU throws uvio_amd::Error with UVIO_HP_E_DEVICE (tests/cpp/facade_odometry_check.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_facade_odometry_compiles_reorders_and_fails_loudly_without_gpu(tmp_path):
    import torch
    lib = os.path.join(ROOT, "uvio_amd", "libuvio_hp.so")
    if not os.path.exists(lib):
        from uvio_amd import build
        build.build_product()
    exe = str(tmp_path / "facade_odometry_check")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "facade_odometry_check.cpp"), "-o", exe, lib,
           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    cfg = os.path.join(ROOT, "configs", "euroc_mav", "estimator_config.yaml")
    # the construction check is the no-device behaviour: hide the devices of a GPU host from the program
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    if torch.cuda.is_available():
        env["HIP_VISIBLE_DEVICES"] = "-1"
    r = subprocess.run([exe, cfg], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "reorder ok" in r.stdout and "code -3" in r.stdout
