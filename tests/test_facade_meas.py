"""The measurement-update part of the C++ facade (include/uvio_hp.hpp): propagate, state_meta, measurement_update,
position_fix, position_fix_jacobian and chi2_95 compile with g++ -Wall -Wextra -Werror, link against
libuvio_hp.so, chi2_95 reads the library's table (and refuses dof 0), and construction without a GPU throws
uvio_amd::Error with UVIO_HP_E_DEVICE (tests/cpp/facade_meas_check.cpp)."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_facade_measurement_update_compiles_links_and_fails_loudly_without_gpu(tmp_path):
    import torch
    lib = os.path.join(ROOT, "uvio_amd", "libuvio_hp.so")
    if not os.path.exists(lib):
        from uvio_amd import build
        build.build_product()
    exe = str(tmp_path / "facade_meas_check")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "facade_meas_check.cpp"), "-o", exe, lib,
           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,--allow-shlib-undefined"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    cfg = os.path.join(ROOT, "configs", "euroc_mav", "estimator_config.yaml")
    # the construction check is the no-device behaviour: hide the devices of a GPU host from the program
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    if torch.cuda.is_available():
        env["HIP_VISIBLE_DEVICES"] = "-1"
    pose = ["0", "0", "0", "1", "1", "2", "3", "0.5", "0", "0"]  # identity attitude: h = p + p_SinI
    r = subprocess.run([exe, cfg] + pose, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = {ln.split()[0]: [float(x) for x in ln.split()[1:]] for ln in r.stdout.splitlines()
             if ln.startswith(("JAC", "CHI2"))}
    assert lines["JAC"][:3] == [1.5, 2.0, 3.0]
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "chi2_095.json")))["table"]
    assert abs(lines["CHI2"][0] - g["1"]) < 1e-9 * g["1"] and abs(lines["CHI2"][1] - g["3"]) < 1e-9 * g["3"]
    assert "code -3" in r.stdout
