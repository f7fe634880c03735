"""uvio_amd/csrc/fast_prop.h (the host math of uvio_hp_fast_state_propagate) and select_imu (imu_math.h) in a
stand-alone program (tests/cpp/fast_prop_check.cpp) against the numpy restatement of
Propagator::fast_state_propagate (tests/fastprop_ref.py, anchored by tests/test_fastprop_ref.py).

Tolerance: 1e-12 relative to the largest entry of each output.  Both sides are FP64 on the host and differ only
in the summation order of products of at most 15 terms."""
import os
import subprocess

import numpy as np
import pytest

import fastprop_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
TOL = 1e-12
SIG = (1.6968e-4, 2.0e-3, 1.9393e-5, 3.0e-3, 9.81)

IDENT = dict(imu_model=0, dw=(1, 0, 0, 1, 0, 1), da=(1, 0, 0, 1, 0, 1), tg=(0,) * 9, q_acc=(0, 0, 0, 1), q_gyro=(0, 0, 0, 1))


def _quat(v):
    return tuple(FR.rot_2_quat(FR.exp_so3(np.array(v, dtype=float))))


def _calib(model):
    """Dw, Da off the identity, a non-zero Tg and both rotations (only one of them is a state variable per model,
    but fast_state_propagate applies both)"""
    return dict(imu_model=model, dw=(1.01, 0.02, -0.015, 0.99, 0.01, 1.02), da=(0.98, -0.01, 0.02, 1.015, -0.02, 0.99),
                tg=(1e-3, -2e-3, 5e-4, 3e-3, -1e-3, 2e-3, -5e-4, 1e-3, 4e-3), q_acc=_quat([0.01, -0.02, 0.015]),
                q_gyro=_quat([-0.02, 0.01, 0.03]))


def _imu(t0, n, dt, seed, w_scale=0.5):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        t = t0 + k * dt
        wm = w_scale * np.array([np.sin(3 * t), np.cos(2 * t), 0.5 * np.sin(5 * t + 1)]) + 1e-3 * w_scale * rng.standard_normal(3)
        am = np.array([0.5 * np.cos(4 * t), 0.3 * np.sin(3 * t), 9.81 + 0.4 * np.sin(2 * t)]) + 1e-2 * rng.standard_normal(3)
        out.append((t, wm, am))
    return out


def _state(seed):
    rng = np.random.default_rng(seed)
    est = np.zeros(16)
    est[0:4] = FR.rot_2_quat(FR.exp_so3(rng.standard_normal(3)))
    est[4:7] = 2 * rng.standard_normal(3)
    est[7:10] = rng.standard_normal(3)
    est[10:13] = 0.01 * rng.standard_normal(3)
    est[13:16] = 0.05 * rng.standard_normal(3)
    A = rng.standard_normal((15, 15))
    cov = 1e-4 * (A @ A.T / 15 + np.eye(15))
    return est, cov


def _cases():
    """(name, calib, t, t_off, imu, queries)"""
    dt = 0.005
    imu = _imu(9.9, 120, dt, 1)  # samples at 9.9, 9.905, ..., 10.495
    on_sample = imu[60][0]
    cs = []
    # both ends interpolated (the state time and the query lie between samples), then a second, chained query
    cs.append(("between_and_chained_kalibr", _calib(0), 10.0012, 0.0, imu, [10.0523, 10.1019]))
    cs.append(("rpng_model", _calib(1), 10.0012, 0.0, imu, [10.0523, 10.1019]))
    # a query exactly on a sample, chained into one between samples
    cs.append(("on_a_sample", _calib(0), 10.0012, 0.0, imu, [on_sample, on_sample + 0.0321]))
    # a non-zero time offset: applied to both ends of the first query, zero afterwards
    cs.append(("time_offset", _calib(1), 10.0012, 0.0137, imu, [10.0523, 10.0871]))
    # |w dt| below exp_so3's (1e-7) and Jl_so3's (1e-6) small-angle thresholds, and between the two
    cs.append(("tiny_rate", IDENT, 10.0012, 0.0, _imu(9.9, 120, dt, 2, w_scale=1e-5), [10.0523]))
    cs.append(("small_rate", _calib(0), 10.0012, 0.0, _imu(9.9, 120, dt, 3, w_scale=1e-4), [10.0523]))
    cs.append(("zero_rate", IDENT, 10.0012, 0.0, [(t, np.zeros(3), a) for t, _, a in imu], [10.0523]))
    # past the newest sample: the stretch branch (Propagator.cpp:358-366)
    cs.append(("past_the_newest", _calib(0), 10.4512, 0.0, imu, [10.5217]))
    # fewer than two readings: ok = 0, outputs and cache untouched; the next query still works
    cs.append(("too_few", _calib(0), 9.5, 0.0, imu[40:], [9.7, 10.2]))
    cs.append(("one_sample", IDENT, 10.0, 0.0, imu[:1], [10.05]))
    cs.append(("no_samples", IDENT, 10.0, 0.0, [], [10.05]))
    return cs


def _fmt(vals):
    return " ".join(repr(float(v)) for v in vals)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    d = tmp_path_factory.mktemp("fast_prop")
    exe = str(d / "fast_prop_check")
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror",
                           "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "uvio_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "fast_prop_check.cpp"), "-o", exe], timeout=300)
    cases = _cases()
    lines = [str(len(cases))]
    for k, (name, cal, t, t_off, imu, queries) in enumerate(cases):
        est, cov = _state(100 + k)
        lines.append(_fmt([cal["imu_model"]] + list(cal["dw"]) + list(cal["da"]) + list(cal["tg"]) + list(cal["q_acc"]) +
                          list(cal["q_gyro"])))
        lines.append(_fmt(SIG))
        lines.append(_fmt([t] + list(est) + list(cov.ravel()) + [t_off]))
        lines.append(str(len(imu)))
        for s in imu:
            lines.append(_fmt([s[0]] + list(s[1]) + list(s[2])))
        lines.append(str(len(queries)))
        lines.append(_fmt(queries))
    inp = d / "cases.txt"
    inp.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = out.stdout.strip().split("\n")
    res, r = {}, 0
    for k, (name, cal, t, t_off, imu, queries) in enumerate(cases):
        res[name] = rows[r:r + len(queries)]
        r += len(queries)
    assert r == len(rows)
    return res


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize("case", [c[0] for c in _cases()])
def test_fast_prop_header_matches_restatement(program, case):
    k, (name, cal, t, t_off, imu, queries) = [(i, c) for i, c in enumerate(_cases()) if c[0] == case][0]
    est, cov = _state(100 + k)
    fp = FR.FastPropagator(FR.Noise(*SIG))
    fp.refresh(t, est, cov, t_off, FR.Calib(**cal))
    n_ok = 0
    for q, row in zip(queries, program[case]):
        tok = row.split()
        v = np.array([float(x) for x in tok[1:]])
        sp, c12, ct, ctoff, e16, c15 = v[0:13], v[13:157].reshape(12, 12), v[157], v[158], v[159:175], v[175:400].reshape(15, 15)
        want = fp.query(imu, q)
        if want is None:
            assert tok[0] == "no", (case, q)
            assert np.all(sp == -777.0) and np.all(c12 == -777.0)  # outputs untouched
        else:
            assert tok[0] == "ok", (case, q)
            n_ok += 1
            figs = {"state_plus": _rel(sp, want[0]), "cov12": _rel(c12, want[1])}
            print(case, q, figs)
            assert max(figs.values()) < TOL, (case, q, figs)
            assert abs(np.linalg.norm(sp[0:4]) - 1) < 1e-12
        # the cache itself: time, offset, estimate and covariance (unchanged after a refused query)
        assert ct == fp.t and ctoff == fp.t_off, (case, q, ct, fp.t)
        assert _rel(e16, fp.est) < TOL and _rel(c15, fp.cov) < TOL, (case, q)
    expect_ok = {"too_few": 1, "one_sample": 0, "no_samples": 0}.get(case, len(queries))
    assert n_ok == expect_ok, (case, n_ok)
